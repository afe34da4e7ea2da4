"""Fine-tuning, host side (no GPU): nmrgnn_amd.finetune against the references of finetune_ref.py, and those references
against hand-worked cases — pattern resolution, the group reduction, the launch plan (exhaustively for L = 1..3), segment
merging with its padding gaps, the float64 grouped Adam and the clip factor."""
import numpy as np
import pytest

import finetune_ref as FR
import node_small_ref as R
from nmrgnn_amd import finetune as FT
from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
from nmrgnn_amd.params import param_shapes


def small_hp(F=64):
    return declare_gnn_space(HyperParameters(atom_feature_size=F, mp_layers=3, fc_layers=2, edge_fc_layers=2))


def package_layout(hp, C):
    """(names, sizes, offsets, numel) as params.ParamStore lays the buffer out"""
    shapes = param_shapes(hp, C)
    sizes = {n: int(np.prod(s)) for n, s in shapes}
    offsets, off = {}, 0
    for n, _ in shapes:
        off = (off + 3) // 4 * 4
        offsets[n] = off
        off += sizes[n]
    return [n for n, _ in shapes], sizes, offsets, (off + 3) // 4 * 4


def test_layout_reference_matches_param_shapes():
    hp = small_hp()
    names, sizes, offsets, numel = package_layout(hp, 7)
    t, off, n = FR.layout(64, hp.get("edge_feature_size"), hp.get("edge_hidden_size"), 2, 3, 2, 7)
    assert [x[0] for x in t] == names and dict(t) == sizes and off == offsets and n == numel
    # C = 7: out/bias has 7 elements, so embed/kernel starts behind a one-element gap
    assert offsets["embed/kernel"] == offsets["out/bias"] + 8


NAMES = package_layout(small_hp(), 7)[0]


def test_groups():
    assert [FT.group_of(n) for n in NAMES] == [FR.group_ref(n) for n in NAMES]
    assert FT.group_of("mp/2/w") == "mp/2" and FT.group_of("edge_fc/1/bias") == "edge_fc" and FT.group_of("out/bias") == "out"
    assert FT.group_names(NAMES) == ["edge_fc", "mp/0", "mp/1", "mp/2", "fc", "out", "embed"]
    assert sorted(FT.group_names(NAMES)) == sorted(FR.all_groups(3))
    assert FT.group_names(["fc/1/bias", "out/kernel", "fc/0/kernel"]) == ["fc", "out"]


def test_resolve_patterns():
    assert FT.resolve(["out/bias"], NAMES) == ["out/bias"]
    assert FT.resolve(["fc"], NAMES) == ["fc/0/kernel", "fc/0/bias", "fc/1/kernel", "fc/1/bias"]
    assert FT.resolve(["mp/2"], NAMES) == ["mp/2/w"]
    assert FT.resolve("mp/*", NAMES) == ["mp/0/w", "mp/1/w", "mp/2/w"]
    assert FT.resolve("*/bias", NAMES) == [n for n in NAMES if n.endswith("bias")]
    # buffer order whatever the order of the patterns; a comma-separated string is several patterns
    assert FT.resolve(["out/*", "edge_fc"], NAMES) == FT.resolve("edge_fc/*, out", NAMES) == \
        [n for n in NAMES if n.startswith(("edge_fc/", "out/"))]
    assert FT.resolve(["*"], NAMES) == NAMES
    for bad in (["mp/3"], ["nothing"], "fc,bogus/*", ["mp"]):
        with pytest.raises(ValueError, match="matches no parameter"):
            FT.resolve(bad, NAMES)
    assert FT.check_names(["out/bias", "mp/1/w"], NAMES) == frozenset({"out/bias", "mp/1/w"})
    for bad in (["fc"], ["out/*"], ["mp/7/w"]):        # names only: no groups, no patterns
        with pytest.raises(ValueError, match="unknown parameter"):
            FT.check_names(bad, NAMES)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_launch_plan_exhaustive(L):
    for groups in FR.subsets(FR.all_groups(L)):
        ref = FR.launch_plan_ref(L, groups)
        plan = FT.launch_plan(L, groups)
        tag = f"L={L} {sorted(groups)}"
        assert plan.fc_run == ref["fc_run"] and plan.fc_dw == ref["fc_dw"], tag
        assert list(reversed(range(plan.mp_stop, L))) == ref["mp_run"], tag
        assert [l for l in reversed(range(plan.mp_stop, L)) if plan.mp_dw[l]] == ref["mp_dw"], tag
        assert plan.embed == ref["embed"] and plan.edge_fc == ref["edge_fc"], tag
        assert (plan.mp_stop < L) == ref["edges"], tag
        want = sorted(groups | {"out"})       # the head's gradient always runs: "out" is always defined
        assert sorted(FT.computed_groups(L, plan)) == want, tag
    full = FT.full_plan(L)
    assert full == FT.Plan(True, True, 0, (True,) * L, True, True)
    with pytest.raises(ValueError):
        FT.launch_plan(L, {f"mp/{L}"})


def test_launch_plan_rules_by_hand():
    """the launch rules of the reference itself on the cases of the GPU test (L = 3)"""
    P = lambda *g: FR.launch_plan_ref(3, g)
    assert P("out") == dict(fc_run=False, fc_dw=False, mp_run=[], mp_dw=[], embed=False, edge_fc=False, edges=False)
    assert P("fc", "out") == dict(fc_run=True, fc_dw=True, mp_run=[], mp_dw=[], embed=False, edge_fc=False, edges=False)
    assert P("mp/2") == dict(fc_run=True, fc_dw=False, mp_run=[2], mp_dw=[2], embed=False, edge_fc=False, edges=True)
    assert P("mp/1", "out") == dict(fc_run=True, fc_dw=False, mp_run=[2, 1], mp_dw=[1], embed=False, edge_fc=False, edges=True)
    assert P("mp/0")["mp_run"] == [2, 1, 0] and P("mp/0")["mp_dw"] == [0]
    assert P("embed") == dict(fc_run=True, fc_dw=False, mp_run=[2, 1, 0], mp_dw=[], embed=True, edge_fc=False, edges=True)
    assert P("edge_fc") == dict(fc_run=True, fc_dw=False, mp_run=[2, 1, 0], mp_dw=[], embed=False, edge_fc=True, edges=True)


def test_scales_first_match_wins():
    sc = FT.scales(NAMES, None, {"mp/1": 0.5, "mp/*": 0.1, "*/bias": 2.0})
    assert sc["mp/1/w"] == 0.5 and sc["mp/0/w"] == sc["mp/2/w"] == 0.1 and sc["fc/0/bias"] == 2.0 and sc["fc/0/kernel"] == 1.0
    assert list(sc) == NAMES
    sc = FT.scales(NAMES, {"out/kernel", "mp/2/w"}, {"mp/*": 0.25})
    assert sc == {"mp/2/w": 0.25, "out/kernel": 1.0}
    for bad in ({"mp/*": -1.0}, {"mp/*": float("nan")}, {"mp/*": float("inf")}):
        with pytest.raises(ValueError, match="finite"):
            FT.scales(NAMES, None, bad)
    with pytest.raises(ValueError, match="matches no parameter"):
        FT.scales(NAMES, None, {"zz/*": 1.0})


@pytest.mark.parametrize("C", [7, 8, 10])
def test_segments_merge_and_gaps(C):
    names, sizes, offsets, numel = package_layout(small_hp(), C)
    cases = [{n: 1.0 for n in names},
             {n: 1.0 for n in names if n.startswith(("fc/", "out/"))},
             {n: (0.1 if n.startswith("mp/") else 1.0) for n in names},
             {"mp/1/w": 1.0}, {"out/bias": 0.5, "embed/kernel": 0.5}, {n: 0.0 for n in names}, {},
             {"fc/0/kernel": 1.0, "fc/0/bias": 0.0, "fc/1/kernel": 1.0}]
    for groups in cases:
        segs = FT.segments(groups, sizes, offsets)
        assert segs == FR.segments_ref(groups, sizes, offsets, numel), groups
        for (b0, e0, _), (b1, e1, _) in zip(segs, segs[1:]):
            assert e0 <= b1 and b0 < e0 and b1 < e1
    full = FT.segments(cases[0], sizes, offsets)
    covered = sum(e - b for b, e, _ in full)
    assert covered == sum(sizes.values())              # the alignment padding belongs to no segment
    # one segment more for every tensor that starts behind a gap (edge_fc's last bias has E = 3 elements: always one)
    gaps = [n for prev, n in zip(names, names[1:]) if offsets[n] != offsets[prev] + sizes[prev]]
    assert len(full) == 1 + len(gaps) and [s[0] for s in full[1:]] == [offsets[n] for n in gaps]
    assert "mp/0/w" in gaps
    if C in (7, 10):      # out/bias [C] ends off a multiple of four: a gap in front of embed/kernel splits the run
        assert full[-1][0] == offsets["embed/kernel"] and full[-2][1] == offsets["out/bias"] + C
        assert full[-1][0] - full[-2][1] == (-C) % 4
    else:
        assert "embed/kernel" not in gaps and full[-1] == (offsets["mp/0/w"], numel, 1.0)
    with pytest.raises(ValueError, match="unknown parameter"):
        FT.segments({"mp/9/w": 1.0}, sizes, offsets)
    with pytest.raises(ValueError, match="finite"):
        FT.segments({"mp/1/w": -0.5}, sizes, offsets)
    many = {f"t{i}": 1 for i in range(70)}
    with pytest.raises(ValueError, match="at most 64"):
        FT.segments({n: 1.0 for n in many}, many, {n: 8 * i for i, n in enumerate(many)})


def test_adam_groups_ref():
    """scale 1 everywhere is adam_ref; a frozen element keeps its input whatever its gradient holds; a power-of-two scale is
    adam_ref at lr * scale; 0.3 scales the update by the float32 product of the rates"""
    rng = np.random.default_rng(3)
    n = 50
    p, g, m = (R.f32(rng.standard_normal(n)) for _ in range(3))
    v = R.f32(rng.standard_normal(n) ** 2)
    args = (1e-3, 0.9, 0.999, 1e-7, 5, 0.5)
    pr, mr, vr, mag = R.adam_ref(p, g, m, v, *args)
    pg, mg, vg, magg, on = FR.adam_groups_ref(p, g, m, v, *args, [(0, n, 1.0)])
    assert on.all() and np.array_equal(pg, pr) and np.array_equal(mg, mr) and np.array_equal(vg, vr)
    assert np.array_equal(magg["upd"], mag["upd"])
    bad = g.copy()
    bad[10:20] = np.nan
    pg, mg, vg, _, on = FR.adam_groups_ref(p, bad, m, v, *args, [(0, 10, 1.0), (10, 20, 0.0), (21, n, 2.0)])
    assert not on[10:21].any() and on[:10].all() and on[21:].all()
    assert np.array_equal(pg[10:21], p[10:21].astype(np.float64)) and np.array_equal(mg[10:21], m[10:21].astype(np.float64))
    assert np.array_equal(pg[:10], pr[:10]) and np.isfinite(pg).all()
    p2 = R.adam_ref(p, g, m, v, 2e-3, *args[1:])[0]
    assert np.allclose(pg[21:], p2[21:], rtol=0, atol=1e-9) and np.array_equal(mg[21:], mr[21:])
    p3 = FR.adam_groups_ref(p, g, m, v, *args, [(0, n, 0.3)])[0]
    lr_t = R.adam_constants(*args[:3], args[4])[0]
    rate = FR.rate_ref(*args[:3], args[4], 0.3)
    assert rate == float(np.float32(lr_t) * np.float32(0.3)) and abs(rate / lr_t - 0.3) < 1e-7
    assert np.allclose(p.astype(np.float64) - p3, (p.astype(np.float64) - pr) * (rate / lr_t), rtol=1e-9, atol=1e-15)


def test_clip_ref():
    g = np.array([3.0, 4.0, 100.0, 12.0], np.float32)
    assert FR.clip_ref(g, 1.0, [(0, 2, 1.0)], 10.0) == (1.0, 5.0)                  # below the threshold: exactly 1
    assert FR.clip_ref(g, 1.0, [(0, 2, 1.0)], 2.5) == (0.5, 5.0)
    assert FR.clip_ref(g, 0.5, [(0, 2, 1.0), (2, 3, 0.0), (3, 4, 0.1)], 1.0) == (1.0 / 6.5, 6.5)      # 1.5, 2, 6: norm 6.5
    assert FR.clip_ref(np.zeros(4, np.float32), 1.0, [(0, 4, 1.0)], 1.0) == (1.0, 0.0)
    f, nrm = FR.clip_ref(np.array([1.0, np.nan], np.float32), 1.0, [(0, 2, 1.0)], 1.0)
    assert f == 1.0 and np.isnan(nrm)
    f, nrm = FR.clip_ref(np.array([1.0, np.inf], np.float32), 1.0, [(0, 2, 1.0)], 1.0)
    assert f == 1.0 and np.isinf(nrm)
    assert FR.clip_ref(g, 1.0, [], 1.0) == (1.0, 0.0)


def test_model_trainable_names_and_cli_usage_errors(tmp_path):
    """pattern resolution at the model and at the command line, where a pattern that selects nothing is a usage error found
    before any record is read (the record file here is not even a record file)"""
    from click.testing import CliRunner
    from nmrgnn_amd.main import main
    from nmrgnn_amd.model import build_GNNModel
    model = build_GNNModel()
    assert model.trainable_names("mp/3,out/*") == ["mp/3/w", "out/kernel", "out/bias"]
    assert model.trainable_names(["fc"]) == [n for n in model.parameter_names() if n.startswith("fc/")]
    with pytest.raises(ValueError, match="matches no parameter"):
        model.trainable_names(["mp/4"])
    rec = tmp_path / "records.npz"
    rec.write_bytes(b"")
    for bad in (["--freeze", "embed/*,nope/*"], ["--lr-scale", "zz/*=0.1"], ["--lr-scale", "mp/*"], ["--lr-scale", "mp/*=-1"],
                ["--freeze", "*"], ["--clipnorm", "0"]):
        res = CliRunner().invoke(main, ["train", str(rec), str(tmp_path / "model"), "1", "--load"] + bad)
        assert res.exit_code == 2 and "Usage" in res.output, (bad, res.output)
