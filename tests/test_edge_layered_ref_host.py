"""CPU checks of tests/edge_layered_ref.py, the float64 statement behind tests/test_gpu_edge_layered_kernels.py: the statement against
the oracle, its gradients against central differences, the exact family's conditions for every case id of the GPU file, the launch
plans against the branch each case is listed under, the counted RBF bound against a float32 emulation, and the rejection of three
wrong emulations by both criteria."""
import numpy as np
import pytest

import edge_layered_ref as R
from edge_layered_ref import ACT, f32
from oracle import nmrgnn_oracle as O
from test_gpu_edge_layered_kernels import BIG_CLAIMS, CASES, CLAIMS, PAIRS, RBF_CASES, big_reference, rbf_case

ACT_NAME = {"none": "linear", "softplus": "softplus", "relu": "relu", "tanh": "tanh"}


# ----------------------------------------------------------------------------------------------------------- statement vs oracle
@pytest.mark.parametrize("act", list(ACT))
@pytest.mark.parametrize("H,Le,E", [(16, 2, 1), (48, 3, 5), (32, 4, 12)])
def test_statement_equals_the_oracle(act, H, Le, E):
    c = R.normal_case(H, Le, E, ACT[act], 37)
    v, _ = R.ref_forward(c, round_tape=False)
    live = c["d_src"] > 0
    x0 = O.rbf_expand(c["d_eff"], c["centers"], c["gap"]) * live[:, None]
    assert np.allclose(v["x0"], x0, rtol=1e-14, atol=0)
    p = {}
    for t in range(Le):
        p[f"edge_fc/{t}/kernel"], p[f"edge_fc/{t}/bias"] = c["Ws"][t], c["bs"][t]
    e, acts = O.edge_fc_block(x0, p, {"fc_activation": ACT_NAME[act], "edge_fc_layers": Le})
    assert np.allclose(v["e"], e * live[:, None], rtol=1e-12, atol=1e-14)
    for t in range(Le - 1):
        assert np.allclose(v["z"][t], acts[t + 1], rtol=1e-12, atol=1e-14), t
    assert (live.any() and not live.all())


@pytest.mark.parametrize("act", list(ACT))
def test_gradients_equal_central_differences(act):
    """dW[t], db[t] of L = sum(e * de) against (L(w + h) - L(w - h)) / 2h in float64, at entries of every layer"""
    H, Le, E, n = 16, 4, 3, 29
    c = R.normal_case(H, Le, E, ACT[act], n)
    v, _ = R.ref_forward(c, round_tape=False)
    g, _ = R.ref_backward(c, v["z"])
    rng = np.random.default_rng(5)
    loss = lambda cc: float((R.ref_forward(cc, round_tape=False)[0]["e"] * cc["de"]).sum())
    h = 1e-6
    for t in range(Le):
        for key, arr in (("dW", c["Ws"]), ("db", c["bs"])):
            for _ in range(6):
                idx = tuple(rng.integers(0, s) for s in arr[t].shape)
                hi, lo = [a.copy() for a in arr], [a.copy() for a in arr]
                hi[t][idx] += h
                lo[t][idx] -= h
                k = "Ws" if key == "dW" else "bs"
                fd = (loss(dict(c, **{k: hi})) - loss(dict(c, **{k: lo}))) / (2 * h)
                scale = np.abs(g[key][t]).max() + 1e-12
                assert abs(fd - g[key][t][idx]) <= 1e-6 * scale, (key, t, idx, fd, g[key][t][idx])


def test_slopes_come_from_the_rounded_tape():
    """the backward takes what it is handed: a tape rounded to float32 changes the gradients by the rounding, not more"""
    c = R.normal_case(32, 3, 2, ACT["tanh"], 50)
    v, _ = R.ref_forward(c)
    a, _ = R.ref_backward(c, v["z"])
    b, mg = R.ref_backward(c, [f32(z) for z in v["z"]])
    for x, y, m in zip(a["dW"], b["dW"], mg["dW"]):
        assert np.any(x != y) and (np.abs(x - y) <= 1e-6 * m + 1e-9).all()


# ------------------------------------------------------------------------------------------------------------------ launch plans
def test_plans():
    assert R.plan(1) == (1, 64) and R.plan(2048) == (1, 2048) and R.plan(2049) == (2, 1088) and R.plan(6145) == (4, 1600)
    assert R.trips(2049)[-2:] == [64, 1] and R.trips(2049).count(64) == 32 and R.trips(6145)[-1] == 1
    assert R.block_ranges(2049) == [(0, 1088), (1088, 2049)]
    nb, rows = R.plan(R.BIG_N)
    assert (nb, rows) == (2048, 2112)
    empty = [b for b, (r0, r1) in enumerate(R.block_ranges(R.BIG_N)) if r0 >= R.BIG_N]
    assert empty == list(range(1986, 2048))
    assert sum(R.trips(R.BIG_N)) == R.BIG_N
    assert R.ew_trips(0) == 0 and R.ew_trips(1) == 1 and R.ew_trips(524288) == 1 and R.ew_trips(524289) == 2
    assert R.ew_trips(131072 * 4) == 1 and R.ew_trips(131073 * 4) == 2              # rbf_kernel at H = 16
    assert R.ew_trips(2047 * 256) == 1 and R.ew_trips(2048 * 256) == 1 and R.ew_trips(2049 * 256) == 2
    assert not R.split_gemm(128, 4095) and R.split_gemm(128, 4097) and R.split_gemm(256, 256) and not R.split_gemm(272, 6145)


@pytest.mark.parametrize("branch", list(CLAIMS))
def test_every_case_reaches_the_branch_it_is_listed_under(branch):
    assert CLAIMS[branch], branch
    for cid in CLAIMS[branch]:
        sp = CASES[cid]
        assert branch in R.branches(sp["H"], sp["Le"], sp["E"], ACT[sp["act"]], sp["n"]), cid


def test_the_table_covers_every_branch():
    """every instantiation, both column counts, every partition shape, every trip count and activation is claimed by some case"""
    need = {f"out<{E}>" for E in range(1, 9)} | {"bwd_col1", "bwd_col2", "nb1", "nb2", "nb4", "nz1", "nz2", "nz4", "rows1088",
                                                 "rows1600", "bwd_last_trip1", "bwd_last_trip63", "bwd_trips_full", "fwd_k1",
                                                 "fwd_wg_full", "fwd_wg_ragged1", "fwd_wg_ragged63", "fwd_wgs>1", "wide", "mask_trips1",
                                                 "mask_trips2", "split", "Le2", "Le3", "Le4", "Le6", "act0", "act1", "act2", "act3"}
    assert need <= set(CLAIMS)
    assert set(BIG_CLAIMS) <= R.branches(16, 2, 1, ACT["relu"], R.BIG_N)
    hs = {(sp["H"], sp["n"]) for sp in CASES.values()}
    for H in (16, 48, 128, 272, 512):
        assert {(H, n) for n in (1, 63, 64, 65, 4097)} <= hs, H                     # edge_out_fwd's row of the table
    for H in (16, 256, 272, 512):
        assert {(H, n) for n in (1, 63, 64, 65, 2048, 2049, 6145)} <= hs, H         # edge_out_bwd's
    assert {(H, n) for H, n in RBF_CASES} >= {(4, 1), (20, 257), (16, 131072), (16, 131073), (128, 257), (512, 257)}
    assert {R.ew_trips(n * (H // 4)) for H, n in RBF_CASES} == {1, 2}


# -------------------------------------------------------------------------------------------------------------- the exact family
EXACT_IDS = [cid for cid, fam in PAIRS if fam == "exact"]


@pytest.mark.parametrize("cid", EXACT_IDS)
def test_exact_family_is_exact_in_float32(cid):
    sp = CASES[cid]
    c = R.make_case("exact", sp["H"], sp["Le"], sp["E"], ACT[sp["act"]], sp["n"], sp["p_dead"])
    v = R.exact_conditions(c)
    dead = c["d_src"] <= 0
    if sp["p_dead"] is None and sp["n"] >= 63:
        assert 0 < dead.mean() < 0.5 and np.isnan(c["d_eff"][dead]).any() and np.signbit(c["d_src"][dead]).any()
        assert all(np.abs(w).max() > 0 for w in v["dW"])
        assert 0.3 < (c["de"] == 0).mean() < 0.7
        assert all(0.15 < (z != 0).mean() < 0.35 for z in c["zs32"])
    if sp["p_dead"] == 1.0:
        assert dead.all()
    if sp["Le"] > 2:                                              # tape layers distinct by construction
        z = R.ref_forward(c)[0]["z"]
        assert all(not np.array_equal(z[a], z[b]) for a in range(len(z)) for b in range(a))


def test_exact_family_big_case():
    """the 4.2 M-row case: float32 numbers, two row orders with the same bits, sums on the integer grid"""
    c, v, _ = big_reference()
    assert c["n"] == R.BIG_N and len(c["d_src"]) == R.BIG_N and c["zs32"][0].shape == (R.BIG_N, 16)
    v2 = R.exact_conditions(c, forward=False, order=np.arange(R.BIG_N)[::-1])
    for a, b in zip(v["dW"] + v["db"], v2["dW"] + v2["db"]):
        assert np.array_equal(a, b)
    assert all(np.abs(w).max() > 0 for w in v["dW"])
    # the rows of the last block with rows, and its neighbours, carry weight: a block dropped or doubled changes the sums
    r0, r1 = R.block_ranges(R.BIG_N)[1985]
    assert r1 == R.BIG_N and (np.asarray(c["de"][r0:r1]) != 0).any()


@pytest.mark.parametrize("H,n", RBF_CASES, ids=str)
def test_rbf_cases(H, n):
    """exact: one-hot in float64 and in the float32 emulation; normal: the emulation of rbf_kernel's roundings stays inside the counted
    bound, and uses a real share of it"""
    d_src, d_eff, centers, gap = rbf_case("exact", H, n)
    ref, _, live = R.rbf(d_src, d_eff, centers, gap)
    assert ((ref == 0) | (ref == 1)).all() and (ref.sum(1) == live).all()
    assert R.same_bits(R.rbf_f32(d_src, d_eff, centers, gap), ref.astype(np.float32))
    d_src, d_eff, centers, gap = rbf_case("normal", H, n)
    ref, arg, live = R.rbf(d_src, d_eff, centers, gap)
    err = np.abs(R.rbf_f32(d_src, d_eff, centers, gap).astype(np.float64) - ref)
    ratio = float((err / R.rbf_bound(ref, arg)).max())
    big = ref > 2.0 ** -100
    print("rbf emulation", H, n, f"all {ratio:.3f} normal-range {float((err / R.rbf_bound(ref, arg))[big].max()) if big.any() else 0:.3f}")
    assert ratio <= 1.0
    if n >= 257:
        assert ratio > 0.05 and live.any() and not live.all() and np.any(d_eff != d_src)


# --------------------------------------------------------------------------------------------------------------- wrong emulations
def _case_and_refs(fam, H, Le, E, act, n):
    c = R.make_case(fam, H, Le, E, ACT[act], n)
    v, mg = R.ref_forward(c)
    zs32 = c["zs32"] if fam == "exact" else [f32(z) for z in v["z"]]
    vb, mgb = R.ref_backward(c, zs32, mz=None if fam == "exact" else mg["z"])
    return c, zs32, dict(v, **vb), dict(mg, **mgb)


def _as_got(v):
    return {k: ([a.astype(np.float32) for a in v[k]] if isinstance(v[k], list) else v[k].astype(np.float32))
            for k in ("e", "z", "dW", "db") if k in v}


@pytest.mark.parametrize("fam", ["exact", "normal"])
def test_the_statement_itself_passes(fam):
    c, zs32, ref, mag = _case_and_refs(fam, 272, 2, 5, "relu", 2049)
    failures = []
    R.hold(fam, _as_got(ref), ref, mag, failures)
    assert not failures


@pytest.mark.parametrize("fam", ["exact", "normal"])
@pytest.mark.parametrize("cid", ["rows-H272-L2-E", "rows-H16-L2-E", "rows-H512-L2-E"])
def test_a_dropped_last_row_of_a_trip_is_rejected(fam, cid):
    """edge_out_bwd_kernel summing rr < nr - 1: dW and db of the output layer lose one row per 64-row trip"""
    for full in [k for k in CASES if k.startswith(cid) and k.endswith(("-n65", "-n2049"))]:
        sp = CASES[full]
        c, zs32, ref, mag = _case_and_refs(fam, sp["H"], sp["Le"], sp["E"], sp["act"], sp["n"])
        wrong, _ = R.ref_backward(c, zs32, mutate="drop_row")
        failures = []
        R.hold(fam, _as_got(wrong), ref, mag, failures)
        names = {f.split(":")[0] for f in failures}
        assert names and names <= {f"dW{sp['Le'] - 1}", f"db{sp['Le'] - 1}"}, (full, failures)


@pytest.mark.parametrize("fam", ["exact", "normal"])
@pytest.mark.parametrize("H,n", [(272, 65), (512, 65), (512, 6145)])
def test_a_skipped_second_weight_column_is_rejected(fam, H, n):
    sp = next(s for s in CASES.values() if s["H"] == H and s["n"] == n and s["Le"] == 2)
    c, zs32, ref, mag = _case_and_refs(fam, H, 2, sp["E"], sp["act"], n)
    wrong, _ = R.ref_backward(c, zs32, mutate="skip_col2")
    failures = []
    R.hold(fam, _as_got(wrong), ref, mag, failures)
    assert [f.split(":")[0] for f in failures] == ["dW1"], failures


@pytest.mark.parametrize("fam", ["exact", "normal"])
def test_reversed_tape_layers_are_rejected(fam):
    """forward: the tape written in reversed layer order; backward: read in reversed order"""
    sp = CASES["tape-H64-L6-E3-relu-n65"]
    c, zs32, ref, mag = _case_and_refs(fam, sp["H"], sp["Le"], sp["E"], sp["act"], sp["n"])
    wrong_f, _ = R.ref_forward(c, mutate="reverse_tape")
    failures = []
    R.hold(fam, _as_got({"e": wrong_f["e"], "z": wrong_f["z"]}), ref, mag, failures)
    assert {f.split(":")[0] for f in failures} == {"z0", "z1", "z3", "z4"}, failures          # z2 is its own mirror image
    wrong_b, _ = R.ref_backward(c, zs32, mutate="reverse_tape")
    failures = []
    R.hold(fam, _as_got(wrong_b), ref, mag, failures)
    assert {"dW0", "db0"} <= {f.split(":")[0] for f in failures}, failures
