"""tests/uncertainty_ref.py checked on the CPU: the closed-form dropout variance against keep-masks drawn with
node_small_ref.dropout_ref, the shifted-sum replica moments against the two-pass reference, replicate_ref's conventions, and
the host refusals of library.shift_uncertainty(position_sigma=).  No GPU."""
import os

import numpy as np
import pytest

import node_small_ref as R
import uncertainty_ref as U

PDB1 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "108M.pdb")


@pytest.mark.parametrize("Fh,C", U.MC_SHAPES)
def test_closed_form_variance_against_drawn_masks(Fh, C):
    """S = 4096 masks per atom, the counters the head kernel draws them from (offset 2^40 + s N Fh / 4): the sample variance
    of delta is within six standard errors of a sample variance, 6 sqrt(2 / (S - 1)) = 0.133 relative, of the formula (the
    excess kurtosis of a scaled Bernoulli(0.8) is 0.25: negligible), and the sample mean within 6 sqrt(var / S) of peaks."""
    S, N = U.MC_S, U.MC_N
    keep = np.float32(0.8)
    rng = np.random.default_rng([U.MC_SEED, Fh, C])
    g, W, b, atoms, std, avg = U.head_data(rng, N, Fh, C)
    peaks, var, _ = U.head_var_ref(g, keep, W, b, atoms, std, avg)
    # replica s draws N * Fh elements from counter offset 2^40 + s * N * Fh / 4: one consecutive run of counters
    m = R.dropout_ref(U.MC_SEED, 1 << 40, keep, S * N * Fh).reshape(S, N, Fh)
    assert set(np.unique(m)) == {np.float32(0), np.float32(1) / keep}
    u = np.einsum("ic,c,fc->if", atoms.astype(np.float64), std.astype(np.float64), W.astype(np.float64))
    t = g.astype(np.float64) * u
    v = atoms.astype(np.float64) @ (std.astype(np.float64) * b + avg)
    delta = np.stack([np.einsum("sif,if->si", m[s0:s0 + 256].astype(np.float64), t) for s0 in range(0, S, 256)]).reshape(S, N) + v
    rel = np.abs(delta.var(axis=0, ddof=1) - var) / var
    z = np.abs(delta.mean(axis=0) - peaks) / np.sqrt(var / S)
    print(f"Fh={Fh} C={C}: variance off by {rel.max():.4f} relative (bound 0.133), mean by {z.max():.2f} standard errors (bound 6)")
    assert rel.max() <= 6.0 * np.sqrt(2.0 / (S - 1))
    assert z.max() <= 6.0


def test_head_var_ref_special_cases():
    rng = np.random.default_rng(3)
    g, W, b, atoms, std, avg = U.head_data(rng, 9, 32, 10, zero_row=4)
    peaks, var, vbar = U.head_var_ref(g, 1.0, W, b, atoms, std, avg)
    assert (var == 0).all() and (vbar == 0).all()
    peaks, var, vbar = U.head_var_ref(g, 0.5, W, b, atoms, std, avg)
    assert var[4] == 0 and peaks[4] == 0 and (np.delete(var, 4) > 0).all() and (var <= vbar * (1 + 1e-12)).all()
    # keep = 0.5: the mask is 0 or 2, delta = sum_f 2 B_f t_f, variance sum_f t_f^2
    u = np.einsum("ic,c,fc->if", atoms.astype(np.float64), std.astype(np.float64), W.astype(np.float64))
    np.testing.assert_allclose(var, ((g * u) ** 2).sum(axis=1), rtol=1e-12)


@pytest.mark.parametrize("kind", ["normal", "nitrogen", "constant"])
@pytest.mark.parametrize("S", [1, 2, 3, 32, 257])
def test_shifted_moments_against_two_pass(kind, S):
    """the kernel's shifted float64 sums, rounded to float32 once: mean within 1 float32 ulp of the two-pass float64 mean,
    variances within 2^-22 relative; exactly 0 for constant columns and for S = 1"""
    N = 257
    mu, v = U.moments_data(np.random.default_rng([S, N, len(kind)]), kind, S, N)
    mean, var, vm = U.ensemble_moments_shifted(mu, v)
    rmean, rvar, rvm = U.ensemble_moments_ref(mu, v)
    assert mean.dtype == np.float32 and var.dtype == np.float32
    assert (np.abs(mean.astype(np.float64) - rmean) <= U.ulp32(rmean)).all()
    assert (np.abs(var.astype(np.float64) - rvar) <= 2.0 ** -22 * rvar).all()
    assert (np.abs(vm.astype(np.float64) - rvm) <= 2.0 ** -22 * rvm).all()
    if kind == "constant" or S == 1:
        assert (var == 0).all() and (mean == mu[0]).all()
    assert U.ensemble_moments_shifted(mu)[2] is None


def test_replicate_ref_conventions():
    from nmrgnn_amd import synth
    b = synth.make_batch(2, 7, 4, 5, 0.3, seed=2)
    N = b["atoms"].shape[0]
    r = U.replicate_ref(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], b["graph_ptr"], 3)
    assert r["atoms"].shape[0] == 3 * N and r["nlist"].shape == (3 * N, 4)
    for s in range(3):
        sl = slice(s * N, (s + 1) * N)
        assert np.array_equal(r["nlist"][sl] - s * N, b["nlist"]) and np.array_equal(r["edges"][sl], b["edges"])
        assert r["nlist"][sl].min() >= s * N and r["nlist"][sl].max() < (s + 1) * N      # padded slots stay inside their replica
    assert r["graph_ptr"].tolist() == [0, 7, 14, 21, 28, 35, 42]
    live = b["edges"] > 0
    rp = np.concatenate([[0], np.cumsum(live.sum(axis=1))])
    c = U.replicate_ref(b["atoms"], b["nlist"][live], b["edges"][live], b["inv_degree"], b["graph_ptr"], 2, row_ptr=rp)
    assert c["row_ptr"].shape == (2 * N + 1,) and c["row_ptr"][N] == rp[-1] and c["row_ptr"][-1] == 2 * rp[-1]
    assert np.array_equal(np.diff(c["row_ptr"]), np.tile(np.diff(rp), 2))
    assert np.array_equal(c["nlist"][rp[-1]:] - N, b["nlist"][live])


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), [0.1, 0.2], np.full((5, 1), 0.1), [0.1, 0.1, -1e-9, 0.1, 0.1],
                                 "wide"])
def test_position_sigma_refusals(bad):
    """a bad sigma raises before the model or the device is touched (the model here is None)"""
    from nmrgnn_amd.library import shift_uncertainty
    atoms = np.eye(10, dtype=np.float32)[[1, 2, 3, 4, 5]]
    pos = np.arange(15, dtype=np.float32).reshape(5, 3)
    with pytest.raises(ValueError, match="position_sigma"):
        shift_uncertainty(None, atoms, pos, samples=4, position_sigma=bad)


def test_position_sigma_accepted_forms():
    from nmrgnn_amd.library import _position_sigma
    assert _position_sigma(0.25, 3).tolist() == [0.25, 0.25, 0.25]
    assert _position_sigma(np.array([0.0, 0.5, 1.0]), 3).dtype == np.float32
    assert _position_sigma(0, 2).tolist() == [0.0, 0.0]


def test_eval_struct_refusals(tmp_path):
    """refused before a model is loaded or a device touched"""
    from click.testing import CliRunner
    from nmrgnn_amd.main import eval_structure, main
    out = str(tmp_path / "o.csv")
    for kw in (dict(uncertainty=4), dict(average=True)):
        with pytest.raises(ValueError, match="--separate"):
            eval_structure((PDB1,), out, separate=True, **kw)
    with pytest.raises(ValueError, match="--position-sigma"):
        eval_structure((PDB1,), out, position_sigma=0.1)
    for flags in (["--uncertainty", "4"], ["--average"]):
        res = CliRunner().invoke(main, ["eval-struct", "--separate", *flags, PDB1, out])
        assert res.exit_code != 0 and "--separate" in res.output
    assert not os.path.exists(out)
