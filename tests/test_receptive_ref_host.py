"""The integer reference of receptive-field pruning (tests/receptive_ref.py), checked without a GPU: hand cases, and the
exactness argument of DESIGN.md §7.17 in float64 — oracle.torch_ref.forward on the whole graph and on the reference-pruned
graph agree at the selected atoms, in the shifts and in the expanded edge gradient, and stop agreeing one hop short."""
import numpy as np
import pytest
import torch

import receptive_ref as R
from helpers import small_batch

TOL = 1e-12         # float64: the two runs do the same arithmetic on the atoms that matter; only summation lengths differ


def test_path_seed_0_three_hops():
    nlist, edges = R.path_case(12)
    seed = np.zeros(12, np.int32)
    seed[0] = 1
    hop = R.hops_padded(nlist, edges, seed, 3)
    assert hop.tolist() == [0, 1, 2, 3] + [-1] * 8
    atoms, inv = R.hand_batch(nlist, edges)
    p = R.prune_padded(atoms, nlist, edges, inv, [0, 12], seed, 3)
    assert p["keep"].tolist() == [0, 1, 2, 3] and p["graph_ptr"].tolist() == [0, 4] and p["graph_index"].tolist() == [0]
    # rows 0..2 keep their live slots, row 3 (hop == hops) has only dead ones; atom 0's second slot was padded
    assert p["nlist"].tolist() == [[1, 0], [0, 2], [1, 3], [0, 0]]
    assert (p["edges"][3] == 0).all() and p["edges"][0, 1] == 0 and (p["edges"][1:3] == edges[1:3]).all()
    assert (p["inv_degree"] == inv[:4]).all()          # copied, not recomputed: row 3 lost its entries, not its degree
    # CSR form of the same
    rp, col, dist, _ = R.to_csr(nlist, edges)
    assert R.hops_csr(rp, col, dist, seed, 3).tolist() == hop.tolist()
    c = R.prune_csr(atoms, rp, col, dist, inv, [0, 12], seed, 3)
    assert c["row_ptr"].tolist() == [0, 1, 3, 5, 5] and c["nlist"].tolist() == [1, 0, 2, 1, 3]
    assert c["row_of"].tolist() == [0, 1, 1, 2, 2]


def test_asymmetric_pair_walks_outgoing_lists():
    nlist, edges = R.asymmetric_case(8)
    s0 = np.zeros(8, np.int32)
    s0[0] = 1
    s5 = np.zeros(8, np.int32)
    s5[5] = 1
    h0 = R.hops_padded(nlist, edges, s0, 4)
    h5 = R.hops_padded(nlist, edges, s5, 4)
    assert h0[5] == -1 and h0.tolist() == [0, 1, -1, -1, -1, -1, -1, -1]     # 5 reads 0; 0 does not read 5
    assert h5[0] == 1 and h5[1] == 2 and h5[5] == 0
    rp, col, dist, _ = R.to_csr(nlist, edges)
    assert R.hops_csr(rp, col, dist, s0, 4).tolist() == h0.tolist()
    assert R.hops_csr(rp, col, dist, s5, 4).tolist() == h5.tolist()


def test_padded_row_does_not_pull_atom_0():
    nlist, edges = R.padded_row_case(6)
    seed = np.zeros(6, np.int32)
    seed[4] = 1
    hop = R.hops_padded(nlist, edges, seed, 4)
    assert hop.tolist() == [-1, -1, -1, 1, 0, -1]        # atom 3's slots are (0, 0.0): atom 0 stays out
    atoms, inv = R.hand_batch(nlist, edges)
    p = R.prune_padded(atoms, nlist, edges, inv, [0, 6], seed, 4)
    assert p["keep"].tolist() == [3, 4] and p["nlist"].tolist() == [[0, 0], [0, 0]] and p["edges"][1, 0] == edges[4, 0]
    # a live distance with a target outside [0, N) is dead too
    nlist[3, 1], edges[3, 1] = 6, 0.2
    assert R.hops_padded(nlist, edges, seed, 4).tolist() == hop.tolist()


def test_ragged_graphs_drop_empty_ones():
    gp = [0, 1, 18, 82]
    rng = np.random.default_rng(2)
    N, K = 82, 4
    nlist = np.zeros((N, K), np.int32)
    edges = np.zeros((N, K), np.float32)
    for g in range(3):
        a, b = gp[g], gp[g + 1]
        if b - a > 1:
            nlist[a:b] = rng.integers(a, b, (b - a, K))
            edges[a:b] = rng.uniform(0.1, 0.3, (b - a, K)) * (rng.random((b - a, K)) > 0.15)
    seed = np.zeros(N, np.int32)
    seed[[30, 70]] = 1
    atoms, inv = R.hand_batch(nlist, edges)
    p = R.prune_padded(atoms, nlist, edges, inv, gp, seed, 2)
    assert p["graph_index"].tolist() == [2] and p["graph_ptr"].tolist() == [0, len(p["keep"])]
    assert p["keep"].min() >= 18 and p["nlist"].min() >= 0 and p["nlist"].max() < len(p["keep"])


# ------------------------------------------------------------------------------------------------------ float64 theorem
def _hp(mp_layers):
    from oracle import nmrgnn_oracle as O
    return O.hypers(atom_feature_size=64, mp_layers=mp_layers)


def _problem(b, frac=0.05, seed=11):
    rng = np.random.default_rng(seed)
    N = b["edges"].shape[0]
    sel = np.sort(rng.choice(N, max(1, int(round(frac * N))), replace=False))
    mask = np.zeros(N, np.int32)
    mask[sel] = 1
    w = np.zeros(N)
    w[sel] = rng.uniform(0.5, 1.5, len(sel))
    y = rng.standard_normal(N) * 2.0
    return sel, mask, w, y


def _run64(atoms, nlist, edges, inv, p, hp, y, w):
    """(peaks, dL/d edges) of L = sum w (peaks - y)^2 in float64"""
    from oracle import torch_ref
    d = torch.tensor(np.asarray(edges, np.float64), requires_grad=True)
    peaks = torch_ref.forward((atoms, nlist, d, inv), p, hp)
    ((peaks - torch.from_numpy(y)) ** 2 * torch.from_numpy(w)).sum().backward()
    return peaks.detach().numpy(), d.grad.numpy()


def _compare(b, mp_layers, hops, form, sel, mask, w, y):
    """(max relative difference of the selected shifts, of the expanded edge gradient) between the whole graph and the
    reference-pruned one"""
    from oracle import nmrgnn_oracle as O
    from oracle import torch_ref
    hp = _hp(mp_layers)
    p = torch_ref.to_torch_params(O.init_params(hp, 10, seed=21, bias_scale=0.1))
    atoms, nlist, edges, inv = b["atoms"], np.asarray(b["nlist"], np.int64), b["edges"], b["inv_degree"]
    peaks, de = _run64(atoms, nlist, edges, inv, p, hp, y, w)
    if form == "padded":
        q = R.prune_padded(atoms, nlist, edges, inv, b["graph_ptr"], mask, hops)
        keep = q["keep"]
        peaks_p, de_p = _run64(q["atoms"], q["nlist"], q["edges"], q["inv_degree"], p, hp, y[keep], w[keep])
        de_x = R.expand_edge_grad_padded(q, nlist, edges, de_p)
        ref_de = de
    else:
        rp, col, dist, _ = R.to_csr(nlist, edges)
        q = R.prune_csr(atoms, rp, col, dist, inv, b["graph_ptr"], mask, hops)
        keep = q["keep"]
        nl_p, ed_p, rows, slot = R.csr_to_padded(q["row_ptr"], q["nlist"], q["edges"].astype(np.float64))
        peaks_p, g = _run64(q["atoms"], nl_p, ed_p, q["inv_degree"], p, hp, y[keep], w[keep])
        de_x = R.expand_edge_grad_csr(q, rp, col, dist, g[rows, slot])
        ref_de = de[edges > 0]
    rows_sel = q["idx"][sel]
    assert (keep[rows_sel] == sel).all()
    dp = np.abs(peaks_p[rows_sel] - peaks[sel]).max() / np.abs(peaks[sel]).max()
    dg = np.abs(de_x - ref_de).max() / np.abs(ref_de).max()
    return dp, dg, len(keep)


@pytest.fixture(scope="module")
def batch():
    return small_batch(3, 60, 16, 10, p_pad=0.15)


@pytest.mark.parametrize("form", ["padded", "csr"])
@pytest.mark.parametrize("mp_layers", [1, 4])
def test_float64_theorem(batch, mp_layers, form):
    sel, mask, w, y = _problem(batch)
    dp, dg, M = _compare(batch, mp_layers, mp_layers, form, sel, mask, w, y)
    print(f"L={mp_layers} {form}: M={M} of {batch['edges'].shape[0]}  peaks {dp:.2e}  edge grad {dg:.2e}")
    assert dp <= TOL and dg <= TOL, (dp, dg)


@pytest.mark.parametrize("form", ["padded", "csr"])
@pytest.mark.parametrize("mp_layers", [1, 4])
def test_one_hop_short_is_not_enough(batch, mp_layers, form):
    """with hops = mp_layers - 1 the selected shifts must change: the field is not larger than needed by accident of the test.
    The graphs are dense (60 atoms, 16 random neighbours), so at four layers the 5 % selection reaches every atom of its
    graphs within two steps and three hops would lose nothing; ONE selected atom with an atom exactly three steps away does
    lose that atom's entries, which its layer-4 value reads through three neighbours."""
    sel, mask, w, y = _problem(batch)
    if mp_layers == 4:
        N = len(mask)
        for i in range(N):
            one = np.zeros(N, np.int32)
            one[i] = 1
            if (R.hops_padded(batch["nlist"], batch["edges"], one, 3) == 3).any():
                break
        sel, mask = np.array([i]), one
        w = mask.astype(np.float64)
    dp, _, _ = _compare(batch, mp_layers, mp_layers - 1, form, sel, mask, w, y)
    print(f"L={mp_layers} hops={mp_layers - 1} {form}: peaks differ by {dp:.2e}")
    assert dp > 1e-6, dp
    assert _compare(batch, mp_layers, mp_layers, form, sel, mask, w, y)[0] <= TOL       # and the full field is still exact


def test_float64_theorem_on_a_band_graph_where_four_hops_prune():
    """the synthetic graphs above are so dense that four hops reach a whole graph; a band graph (i +- 1, i +- 2) keeps
    the field of one atom to 17 of 200 atoms at mp_layers = 4"""
    N, K = 200, 4
    nlist = np.zeros((N, K), np.int32)
    edges = np.zeros((N, K), np.float32)
    rng = np.random.default_rng(5)
    for i in range(N):
        js = [j for j in (i - 2, i - 1, i + 1, i + 2) if 0 <= j < N]
        nlist[i, :len(js)] = js
        edges[i, :len(js)] = rng.uniform(0.1, 0.3, len(js))
    atoms, inv = R.hand_batch(nlist, edges, C=10)
    b = dict(atoms=atoms, nlist=nlist, edges=edges, inv_degree=inv, graph_ptr=[0, N])
    sel = np.array([100])
    mask = np.zeros(N, np.int32)
    mask[sel] = 1
    w = mask.astype(np.float64)
    y = rng.standard_normal(N)
    for form in ("padded", "csr"):
        dp, dg, M = _compare(b, 4, 4, form, sel, mask, w, y)
        assert M == 17 and dp <= TOL and dg <= TOL, (M, dp, dg)
        assert _compare(b, 4, 3, form, sel, mask, w, y)[0] > 1e-6


def test_selection_is_validated_on_the_host():
    """GraphBatch.restrict's reading of ``select``: masks and index arrays give the same seeds; bad ones raise before any
    device work"""
    from nmrgnn_amd.graph import _select_seed
    cpu = torch.device("cpu")
    mask = np.zeros(9, bool)
    mask[[2, 7]] = True
    for sel in (mask, mask.astype(np.float32), [7, 2], np.array([2, 7], np.int32), torch.tensor([7, 2]),
                torch.from_numpy(mask)):
        seed, idx = _select_seed(sel, 9, cpu)
        assert seed.dtype == torch.int32 and seed.tolist() == mask.astype(int).tolist() and idx.tolist() == [2, 7]
    for bad in ([9], [-1], [3, 3], np.zeros(9, bool), np.ones(8, bool), np.ones((3, 3), bool), [0.5, 2.0], [],
                mask.astype(np.int64)):         # integers are indices whatever their values: here 0 seven times
        with pytest.raises(ValueError):
            _select_seed(bad, 9, cpu)
