"""Per-name metrics on the GPU (ng_name_metrics; nmrgnn_amd/metrics.py): the reference's known answer
(tests/test_nmrgnn.py:111-137 of the reference, restated), a float64 NumPy restatement of nmrgnn/metrics.py on the same
fp32 inputs, the edge cases, determinism, accumulation, and the wiring into Trainer, TrainStepReplay and
GNNModel.evaluate."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (mean, std) of the shifts per element, as the standards give them: H, C, N
SHIFTS = [(5.63, 6.040644), (126.0, 10.603463), (118.955, 50.941216)]


def _np_metric(m, y, names, w, pred):
    """nmrgnn/metrics.py in float64 NumPy, with the edge cases of nmrgnn_amd.metrics"""
    from nmrgnn_amd import NameCorr, NameCount, NameRMSD
    ln = np.atleast_1d(np.asarray(m.label_idx, np.int32))
    mask = np.asarray(w, np.float64) * np.any(np.asarray(names)[:, None] == ln[None, :], axis=-1)
    x, p = np.asarray(y, np.float64), np.asarray(pred, np.float64)
    S = mask.sum()
    if isinstance(m, NameCount):
        return S
    if isinstance(m, NameRMSD):
        return math.sqrt((mask * (x - p) ** 2).sum() / S) if S != 0 else 0.0
    assert isinstance(m, NameCorr)
    if S == 0:
        return math.nan
    xm, ym = (mask * x).sum() / S, (mask * p).sum() / S
    xm2, ym2 = (mask * x * x).sum() / S, (mask * p * p).sum() / S
    cov = (mask * (x - xm) * (p - ym)).sum()
    vx, vy = xm2 - xm ** 2, ym2 - ym ** 2
    vx = 0.0 if vx <= 1e-12 * abs(xm2) else vx          # a variance that is zero after rounding is zero
    vy = 0.0 if vy <= 1e-12 * abs(ym2) else vy
    den = S * math.sqrt(vx * vy)
    return cov / den if den != 0 else 0.0


def _check(got, metrics, y, names, w, pred):
    from nmrgnn_amd import NameCorr
    for m in metrics:
        want = _np_metric(m, y, names, w, pred)
        if isinstance(m, NameCorr):
            if math.isnan(want):
                assert math.isnan(got[m.name]), m.name
            else:
                assert abs(got[m.name] - want) <= 1e-9, (m.name, got[m.name], want)
        else:
            assert got[m.name] == pytest.approx(want, rel=1e-10, abs=0), (m.name, got[m.name], want)


def _data(N, n_names, rng):
    """fp32 shifts around the H / C / N standards, predictions near them, non-binary weights with zeros, name ids that
    include ids outside the table and negative ones"""
    el = rng.integers(0, 3, N)
    mu = np.array([s[0] for s in SHIFTS])[el]
    sd = np.array([s[1] for s in SHIFTS])[el]
    y = (mu + sd * rng.standard_normal(N)).astype(np.float32)
    pred = (y + 0.3 * sd * rng.standard_normal(N) + 0.1 * sd).astype(np.float32)
    w = rng.uniform(0.0, 2.0, N).astype(np.float32)
    w[rng.random(N) < 0.2] = 0.0
    names = rng.integers(-3, n_names + 6, N).astype(np.int32)
    return y, names, w, pred


def _metrics(K, n_names, rng):
    from nmrgnn_amd import NameCorr, NameCount, NameRMSD
    kinds = [NameRMSD, NameCorr, NameCount]
    out = []
    for k in range(K):
        ids = sorted(set(rng.integers(0, n_names, rng.integers(1, 7)).tolist()))
        out.append(kinds[k % 3](ids, name=f"m{k}"))
    return out


def _dev(x, dev, dt=torch.float32):
    return torch.as_tensor(x).to(device=dev, dtype=dt).contiguous()


def test_reference_known_answer(gpu_device):
    """the reference's TestMetrics.test_name_rmsd inputs and answers, through the reference's surface (NumPy inputs)"""
    from nmrgnn_amd import NameRMSD, type_mask
    E = {'name': {'ALA-N': 4, 'GLU-N': 2, 'GLU-H': 3}}
    y = np.stack([np.zeros(5), [4., 3, 3, 2, 4], np.ones(5)], axis=1).astype(np.float32)
    y_pred = np.zeros((5,))
    y_pred[1] = 5
    nm = NameRMSD(type_mask(r'.*\-H', E, regex=True))
    nm.update_state(y, y_pred)
    np.testing.assert_allclose(nm.result(), np.sqrt(5.0 ** 2 / 2))
    nm = NameRMSD(type_mask(r'GLU-H', E, regex=True))
    nm.update_state(y, y_pred)
    np.testing.assert_allclose(nm.result(), np.sqrt(5.0 ** 2 / 2))
    y_pred[:] = 0
    y_pred[-2] = 5
    nm = NameRMSD(type_mask(r'GLU\-.*', E, regex=True))
    nm.update_state(y, y_pred)
    np.testing.assert_allclose(nm.result(), np.sqrt(5 ** 2 / 3))
    # device tensors in, the same answer
    nm.update_state(torch.from_numpy(y).to(gpu_device), torch.from_numpy(y_pred).to(gpu_device))
    np.testing.assert_allclose(nm.result(), np.sqrt(5 ** 2 / 3))
    nm.reset_states()
    assert nm.result() == 0.0


@pytest.mark.parametrize("N", [1, 255, 257, 131072])
@pytest.mark.parametrize("K", [1, 15, 32])
def test_against_numpy(gpu_device, N, K):
    from nmrgnn_amd import NameMetrics
    rng = np.random.default_rng(N * 100 + K)
    n_names = 40
    metrics = _metrics(K, n_names, rng)
    y, names, w, pred = _data(N, n_names, rng)
    nm = NameMetrics(metrics)
    nm.update(_dev(pred, gpu_device), _dev(y, gpu_device), _dev(w, gpu_device), _dev(names, gpu_device, torch.int32))
    _check(nm.results(), metrics, y, names, w, pred)
    # the reference's surface: y_true[N, 3] = [shift, name id, weight], one metric at a time
    yt = np.stack([y, names.astype(np.float32), w], axis=1)
    for m in metrics[:3]:
        m.update_state(yt, pred)
        _check({m.name: m.result()}, [m], y, names, w, pred)


def test_no_atoms(gpu_device):
    from nmrgnn_amd import NameMetrics, NameRMSD
    e = lambda dt=torch.float32: torch.empty(0, dtype=dt, device=gpu_device)
    nm = NameMetrics([NameRMSD([1, 2])])
    nm.update(_dev(np.ones(3, np.float32), gpu_device), _dev(np.zeros(3, np.float32), gpu_device),
              _dev(np.ones(3, np.float32), gpu_device), _dev(np.array([1, 2, 3], np.int32), gpu_device, torch.int32))
    nm.update(e(), e(), e(), e(torch.int32))
    assert torch.count_nonzero(nm.moments).item() == 0
    acc = NameMetrics([NameRMSD([1, 2])], accumulate=True)
    acc.update(_dev(np.ones(3, np.float32), gpu_device), _dev(np.zeros(3, np.float32), gpu_device),
               _dev(np.ones(3, np.float32), gpu_device), _dev(np.array([1, 2, 3], np.int32), gpu_device, torch.int32))
    before = acc.moments.clone()
    acc.update(e(), e(), e(), e(torch.int32))
    assert torch.equal(acc.moments, before)


def test_edge_cases(gpu_device):
    from nmrgnn_amd import NameCorr, NameCount, NameMetrics, NameRMSD
    rng = np.random.default_rng(5)
    N = 4096
    y, names, w, pred = _data(N, 20, rng)
    # an empty class: ids no atom carries
    empty = [NameRMSD([100], name='rmsd'), NameCount([100], name='count'), NameCorr([100], name='r')]
    nm = NameMetrics(empty)
    nm.update(_dev(pred, gpu_device), _dev(y, gpu_device), _dev(w, gpu_device), _dev(names, gpu_device, torch.int32))
    got = nm.results()
    assert got['rmsd'] == 0.0 and got['count'] == 0.0 and math.isnan(got['r'])
    # constant predictions (and constant labels) give r = 0
    cls = [NameCorr(list(range(20)), name='r')]
    nm = NameMetrics(cls)
    nm.update(_dev(np.full(N, 118.3, np.float32), gpu_device), _dev(y, gpu_device), _dev(w, gpu_device),
              _dev(names, gpu_device, torch.int32))
    assert nm.results()['r'] == 0.0
    nm.update(_dev(pred, gpu_device), _dev(np.full(N, 5.63, np.float32), gpu_device), _dev(w, gpu_device),
              _dev(names, gpu_device, torch.int32))
    assert nm.results()['r'] == 0.0
    # ids outside the table and negative ids are in no class, even when a metric lists a negative id
    nm = NameMetrics([NameCount([-1, -2, -3], name='neg'), NameCount([0], name='zero')])
    nm.update(_dev(pred, gpu_device), _dev(y, gpu_device), _dev(w, gpu_device), _dev(names, gpu_device, torch.int32))
    got = nm.results()
    assert got['neg'] == 0.0
    assert got['zero'] == pytest.approx(float(w.astype(np.float64)[names == 0].sum()), rel=1e-12)


def test_deterministic(gpu_device):
    from nmrgnn_amd import NameMetrics
    rng = np.random.default_rng(9)
    metrics = _metrics(15, 40, rng)
    args = [_dev(a, gpu_device, dt) for a, dt in zip(_data(131072, 40, rng)[::-1], [torch.float32, torch.float32,
                                                                                    torch.int32, torch.float32])]
    pred, w, names, y = args
    a, b = NameMetrics(metrics), NameMetrics(metrics)
    a.update(pred, y, w, names)
    b.update(pred, y, w, names)
    torch.cuda.synchronize()
    assert torch.equal(a.moments, b.moments)


def test_accumulate(gpu_device):
    from nmrgnn_amd import NameMetrics
    rng = np.random.default_rng(11)
    metrics = _metrics(15, 40, rng)
    parts = [_data(n, 40, rng) for n in (1000, 70000, 333)]
    t = lambda p: (_dev(p[3], gpu_device), _dev(p[0], gpu_device), _dev(p[2], gpu_device), _dev(p[1], gpu_device, torch.int32))
    acc, last, one = NameMetrics(metrics, accumulate=True), NameMetrics(metrics), NameMetrics(metrics)
    for p in parts:
        acc.update(*t(p))
        last.update(*t(p))
    cat = tuple(np.concatenate([p[i] for p in parts]) for i in range(4))
    one.update(*t(cat))
    torch.testing.assert_close(acc.moments, one.moments, rtol=1e-12, atol=0)
    _check(acc.results(), metrics, *cat)
    alone = NameMetrics(metrics)
    alone.update(*t(parts[-1]))
    assert torch.equal(last.moments, alone.moments)
    acc.reset_states()
    assert torch.count_nonzero(acc.moments).item() == 0
    assert all(v == 0.0 for v in acc.results().values())


def _hp(F=64):
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    return declare_gnn_space(HyperParameters(atom_feature_size=F, edge_feature_size=3, edge_hidden_size=128, mp_layers=4,
                                             fc_layers=4, edge_fc_layers=4))


def _labels(N, rng, n_names=40):
    y, names, w, _ = _data(N, n_names, rng)
    return y, names, w


def test_trainer_step_with_metrics(gpu_device):
    from nmrgnn_amd import synth
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.graph import GraphBatch
    from nmrgnn_amd.train import Trainer
    rng = np.random.default_rng(21)
    metrics = _metrics(15, 40, rng)
    dev = gpu_device
    ea, eb = Engine(_hp(), 10, device=dev, seed=77), Engine(_hp(), 10, device=dev, seed=77)
    ta, tb = Trainer(ea, lr=1e-3, metrics=metrics), Trainer(eb, lr=1e-3)
    seen = {}
    orig = ea.backward

    def backward(*a, **kw):           # the training-mode peaks of the step, before backward() drops the tape
        seen['peaks'] = ea.tape.peaks.clone()
        return orig(*a, **kw)

    ea.backward = backward
    for step in range(2):
        b = synth.make_batch(4, 64, 16, 10, 0.05, seed=300 + step)
        y, names, w = _labels(b["atoms"].shape[0], rng)
        gb = lambda: GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
        la = ta.step(gb(), _dev(y, dev), _dev(w, dev), names=_dev(names, dev, torch.int32))
        lb = tb.step(gb(), _dev(y, dev), _dev(w, dev))
        torch.cuda.synchronize()
        assert torch.equal(la, lb), step
        assert torch.equal(ea.params.flat, eb.params.flat), step
        assert torch.equal(ea.adam_m, eb.adam_m) and torch.equal(ea.adam_v, eb.adam_v)
        _check(ta.metric_results(), metrics, y, names, w, seen['peaks'].cpu().numpy())


def test_train_step_replay_with_metrics(gpu_device):
    from nmrgnn_amd import NameMetrics, synth
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.graph import GraphBatch
    from nmrgnn_amd.replay import TrainStepReplay
    from nmrgnn_amd.train import Trainer
    rng = np.random.default_rng(31)
    metrics = _metrics(15, 40, rng)
    dev = gpu_device
    steps = []
    for s in range(3):
        b = synth.make_batch(1, 256, 16, 10, 0.05, seed=700 + s)
        steps.append((b, _labels(256, rng)))
    ea, eb = Engine(_hp(), 10, device=dev, seed=78), Engine(_hp(), 10, device=dev, seed=78)
    ta = Trainer(ea, lr=1e-3, metrics=NameMetrics(metrics, accumulate=True))
    tb = Trainer(eb, lr=1e-3, metrics=NameMetrics(metrics, accumulate=True))
    b0, (y0, n0, w0) = steps[0]
    raw = lambda b: (b["atoms"], b["nlist"], b["edges"], b["inv_degree"])
    rp = TrainStepReplay(tb, raw(b0), y0, w0, graph_ptr=b0["graph_ptr"], names=n0)
    assert tb.metrics.updates == 0 and torch.count_nonzero(tb.metrics.moments).item() == 0   # warm-up left no trace
    for b, (y, names, w) in steps:
        ta.step(GraphBatch(*raw(b), graph_ptr=b["graph_ptr"], device=dev), _dev(y, dev), _dev(w, dev),
                names=_dev(names, dev, torch.int32))
        rp.step(raw(b), y, w, names=names)
        torch.cuda.synchronize()
        assert torch.equal(ea.params.flat, eb.params.flat)
        assert torch.equal(ta.metrics.moments, tb.metrics.moments)
    assert ta.metric_results().keys() == tb.metric_results().keys()


def test_evaluate(gpu_device):
    from nmrgnn_amd import build_GNNModel, synth
    from nmrgnn_amd.graph import GraphBatch
    from nmrgnn_amd.hypers import HyperParameters
    rng = np.random.default_rng(41)
    names_table = {}
    for res in ("ALA", "GLY", "SER"):
        for atom in ("N", "H", "CA", "HA", "C", "CB", "HB2"):
            names_table[f"{res}-{atom}"] = len(names_table)
    names_table.update({"DFT-C": len(names_table), "DFT-H": len(names_table) + 1, "MB-C": len(names_table) + 2,
                        "MB-H": len(names_table) + 3})
    model = build_GNNModel(HyperParameters(atom_feature_size=64), embeddings={'name': names_table}, device=gpu_device)
    assert len(model.metrics) == 15
    data = []
    for G, n in ((2, 64), (3, 100), (1, 200)):
        b = synth.make_batch(G, n, 16, 10, 0.05, seed=900 + G)
        N = b["atoms"].shape[0]
        y, names, w = _labels(N, rng, n_names=len(names_table))
        yt = np.stack([y, names.astype(np.float32), w], axis=1)
        data.append(((b["atoms"], b["nlist"], b["edges"], b["inv_degree"]), yt, b["graph_ptr"]))
    got = model.evaluate(data)
    peaks, ys, loss = [], [], []
    for (inp, yt, gp) in data:
        p = model(GraphBatch(*inp, graph_ptr=gp, device=gpu_device)).cpu().numpy()
        peaks.append(p)
        ys.append(yt)
        for g in range(len(gp) - 1):
            sl = slice(gp[g], gp[g + 1])
            wg = yt[sl, 2].astype(np.float64)
            d = yt[sl, 0].astype(np.float64) - p[sl].astype(np.float64)
            loss.append((wg * d * d).sum() / wg.sum())
    ycat, pcat = np.concatenate(ys), np.concatenate(peaks)
    _check(got, model.metrics, ycat[:, 0], ycat[:, 1].astype(np.int32), ycat[:, 2], pcat)
    assert got['loss'] == pytest.approx(float(np.mean(loss)), rel=1e-6)
    assert set(got) == {'loss'} | {m.name for m in model.metrics}
