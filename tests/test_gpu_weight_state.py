"""State derived from the weights that outlives a call — the library's packed weight images (ng_ctx::wimg, refreshed behind
ng_adam_step), Engine._wgen with the edge-function table kept for frozen weights and ShiftRestraint's refusal, and the chains
recorded by replay.py — against engines that keep none of it.

The reference of every test is (a) an eager twin driven through the same operations with Trainer(cache_images=False), not
frozen, never replayed: it packs every image in front of its use; or (b) a fresh Engine holding the current parameters that
makes the same call as its first call, with the same freeze setting (a table built for reuse covers a quarter more range on
either side than one built for a single call, so the freeze setting is part of "the same call").  The criterion is
torch.equal: "the images are the same bits whichever launch builds them", "the replayed chain gives the bits of the eager
chain".  One engine per scenario; the shared context is left unfrozen, disarmed and with deferral off.

  1  replayed steps on a frozen engine: the table (and, with NG_EDGE_GRAD_TABLE=1, the Jacobian table) kept over calls must not
     survive them
  2  ShiftRestraint refuses after replayed steps as after eager ones
  3  weights out of the fp16 piece range and back while steps are replayed: the image flag pair comes down again
  4  ForwardReplay refuses after an announced weight change; a new one gives the eager forward
  5  TrainStepReplay refuses after an announced change until one eager step has rebuilt the images
  5b another engine takes the device's cache over, then an eager step of a shape that keeps fewer images: the recorded chain
     of the larger shape must not multiply with images nobody rebuilt (F = 256: loss 684.97 against the twin's 73.25 before
     TrainStepReplay._refresh)
  6  seeded sequences of nine kinds of operation (weight_cache_cases.sequence)

On scratch builds: without the _wgen advance of a replayed step 1, 2 and 6 fail; with the parent's flag logic 3
and the F = 64 sequences."""
import os

import numpy as np
import pytest
import torch

import weight_cache_cases as wc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _hp(F):
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    return declare_gnn_space(HyperParameters(atom_feature_size=F, edge_feature_size=3, edge_hidden_size=128, mp_layers=4,
                                             fc_layers=4, edge_fc_layers=4))


def _graphs(n, atoms=256, K=16, C=10):
    from nmrgnn_amd import synth
    out = []
    for g in range(n):
        b = synth.make_batch(1, atoms, K, C, 0.05, seed=700 + g)
        out.append(((b["atoms"], b["nlist"], b["edges"], b["inv_degree"]), b["graph_ptr"], b["y"], b["w"]))
    return out


def _batch(dev, n_graphs, n_atoms, seed):
    from nmrgnn_amd import synth
    from nmrgnn_amd.graph import GraphBatch
    b = synth.make_batch(n_graphs, n_atoms, 16, 10, 0.05, seed=seed)
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
    return gb, _t(dev, b["y"]), _t(dev, b["w"])


def _t(dev, a):
    return torch.as_tensor(np.asarray(a)).to(device=dev, dtype=torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _eager(tr, dev, g):
    from nmrgnn_amd.graph import GraphBatch
    raw, gp, y, w = g
    return tr.step(GraphBatch(*raw, graph_ptr=gp, device=dev), _t(dev, y), _t(dev, w)).clone()


def _fresh(eng, frozen):
    """an engine that has kept nothing: the parameters of `eng` as they are now, its attributes, its freeze setting"""
    from nmrgnn_amd.engine import Engine
    e = Engine(eng.hp, eng.C, device=eng.device, seed=1)
    e.params.flat.copy_(eng.params.flat)
    e.peak_std.copy_(eng.peak_std)
    e.peak_avg.copy_(eng.peak_avg)
    for name in ("edge_table", "edge_table_min_edges", "edge_table_tol", "edge_grad_table", "edge_grad_table_tol", "use_live_edges"):
        setattr(e, name, getattr(eng, name))
    e.freeze_weights(frozen)
    return e


def _release(*engines):
    """the shared context as the next test expects it"""
    from nmrgnn_amd import _lib
    ctx = _lib.get_context(0)
    for e in engines:
        e.freeze_weights(False)
    ctx.lib.ng_replay_arm(ctx.handle, 0)
    ctx.lib.ng_weights_frozen(ctx.handle, 0)
    ctx.lib.ng_defer_reductions(ctx.handle, None, 0)
    torch.cuda.synchronize()


def _moved(sd, k=1):
    """another set of weights of the same size: every entry moved by a few per cent, none by the same amount"""
    out = {}
    for j, (name, v) in enumerate(sorted(sd.items())):
        i = np.arange(v.size, dtype=np.float64).reshape(v.shape)
        out[name] = (v * 0.97 + 0.004 * np.cos(0.37 * i + j + k)).astype(np.float32)
    return out


def _excursion(sd, back):
    sd = {k: v.copy() for k, v in sd.items()}
    for name, idx, val in wc.EXCURSION:
        sd[name][idx] = 0.25 if back else val
    return sd


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("grad_table", [False, True], ids=["values", "jacobian"])
@pytest.mark.parametrize("F", [64, 256])
def test_replayed_steps_void_the_tables_kept_for_frozen_weights(gpu_device, monkeypatch, F, grad_table):
    """a frozen engine keeps the edge-function table over calls under the key (_wgen, T, E).  The replay is built FIRST (its
    warm-up and capture advance _wgen on the host); two validation forwards then keep a table; three replayed steps move the
    weights without running Engine.adam_step.  The forward behind them must be that of a fresh frozen engine holding the
    current weights — and not the one from before the steps.  `jacobian`: the same through forward(keep_tape="inputs") +
    backward(param_grad=False, edge_grad=...) with NG_EDGE_GRAD_TABLE=1, which keeps the Jacobian table beside the values'."""
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.replay import TrainStepReplay
    from nmrgnn_amd.train import Trainer
    dev = gpu_device
    if grad_table:
        monkeypatch.setenv("NG_EDGE_GRAD_TABLE", "1")
    eng = Engine(_hp(F), 10, device=dev, seed=31)
    assert eng.edge_grad_table == grad_table
    eng.edge_table_min_edges = 0          # the small batch takes the device-guarded table
    eng.freeze_weights(True)
    tr = Trainer(eng, lr=2e-3)
    val, _, _ = _batch(dev, 4, 64, seed=21)
    dp = _t(dev, np.cos(np.arange(val.N)))

    def call(e):
        if not grad_table:
            return [e.forward(val).clone()]
        p = e.forward(val, keep_tape="inputs").clone()
        g = torch.full_like(val.edges, float("nan"))
        e.backward(dp, param_grad=False, edge_grad=g)
        return [p, g]

    try:
        gs = _graphs(4)
        raw0, gp0, y0, w0 = gs[0]
        rp = TrainStepReplay(tr, raw0, y0, w0, graph_ptr=gp0)
        call(eng)
        before = call(eng)
        assert eng._table_cache is not None and (not grad_table or "J_all" in eng._table_cache)
        for s in range(3):
            raw, gp, y, w = gs[s + 1]
            rp.step(raw, y, w)
        after = call(eng)
        ref = call(_fresh(eng, True))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(after[0]).all())
        assert not torch.equal(after[0], before[0])
        assert _same(after, ref)
    finally:
        tr.close()
        _release(eng)


# ------------------------------------------------------------------------------------------------------------------ 2
def _structure():
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    s = read_pdb(os.path.join(HERE, "data", "108M.pdb"))
    return atoms_onehot(s.elements), np.asarray(s.frames[0], np.float32)


@pytest.mark.parametrize("F", [64, 256])
def test_shift_restraint_refuses_after_replayed_steps(gpu_device, F):
    """the refusal of a call "after the model's weights changed (a training step or a load)" holds for replayed steps as for
    eager ones: the restraint's captured chain holds no pack launch"""
    from helpers import make_hp
    from nmrgnn_amd.library import ShiftRestraint
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.replay import TrainStepReplay
    from nmrgnn_amd.standards import load_standards
    from nmrgnn_amd.train import Trainer
    atoms, p = _structure()
    model = GNNModel(make_hp(atom_feature_size=F), load_standards(), device=gpu_device, seed=3)
    model.build(atoms.shape[1])
    eng = model.engine
    tr = Trainer(eng, lr=1e-3)
    try:
        gs = _graphs(3, C=atoms.shape[1])
        raw0, gp0, y0, w0 = gs[0]
        rp = TrainStepReplay(tr, raw0, y0, w0, graph_ptr=gp0)
        targets = np.zeros(p.shape[0], np.float32)
        r = ShiftRestraint(model, atoms, targets)
        e, f = r(p)
        assert bool(torch.isfinite(f).all())
        msgs = []
        for replayed in (False, True):
            raw, gp, y, w = gs[1 + replayed]
            if replayed:
                rp.step(raw, y, w)
                rp.step(raw, y, w)
            else:
                _eager(tr, gpu_device, gs[1])
            with pytest.raises(ValueError, match="weights changed") as info:
                r(p)
            msgs.append(str(info.value))
            r = ShiftRestraint(model, atoms, targets)       # a new restraint sees the new weights
            assert bool(torch.isfinite(r(p)[1]).all())
        assert msgs[0] == msgs[1]
    finally:
        tr.close()
        _release(eng)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_replayed_steps_return_to_the_piece_bodies_when_weights_come_back_into_range(gpu_device):
    """F = 64.  Capture; three weights leave the piece range (load, one eager step, two replayed steps: the f32-input bodies);
    they come back to 0.25 (load, one eager step, three replayed steps: the split-operand bodies again, as in the eager twin).
    The recorded repack launch carries ONE version argument for all its replays: the flag pair of an image could not be
    lowered by a launch with the version that raised it."""
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.replay import TrainStepReplay
    from nmrgnn_amd.train import Trainer
    dev = gpu_device
    gs = _graphs(8)
    ea, eb = Engine(_hp(64), 10, device=dev, seed=92), Engine(_hp(64), 10, device=dev, seed=92)
    ta, tb = Trainer(ea, lr=1e-3), Trainer(eb, lr=1e-3, cache_images=False)
    try:
        raw0, gp0, y0, w0 = gs[0]
        rp = TrainStepReplay(ta, raw0, y0, w0, graph_ptr=gp0)
        step = 0
        for back, replays in ((False, 2), (True, 3)):
            sd = _excursion(eb.params.state_dict(), back)
            ea.params.load_state_dict(sd)
            eb.params.load_state_dict(sd)
            for k in range(1 + replays):
                g = gs[step % len(gs)]
                la = _eager(ta, dev, g) if k == 0 else rp.step(g[0], g[2], g[3]).clone()
                lb = _eager(tb, dev, g)
                torch.cuda.synchronize()
                assert torch.equal(la, lb), (back, k, float(la), float(lb))
                assert torch.equal(ea.params.flat, eb.params.flat), (back, k)
                step += 1
            if not back:
                assert float(ea.params.flat.abs().max()) > 256.0
        assert float(ea.params.flat.abs().max()) < 255.0 and bool(torch.isfinite(ea.params.flat).all())
        assert torch.equal(ea.adam_m, eb.adam_m) and torch.equal(ea.adam_v, eb.adam_v)
    finally:
        ta.close()
        tb.close()
        _release(ea, eb)


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("F", [64, 256])
def test_forward_replay_refuses_after_an_announced_change(gpu_device, F):
    """ForwardReplay on a frozen engine, then params.load_state_dict: the chain holds no pack launch and reads the table of the
    old weights, so a call raises ValueError instead of answering with them; a new ForwardReplay gives the eager forward"""
    from helpers import make_hp
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.replay import ForwardReplay
    dev = gpu_device
    atoms, p = _structure()
    rng = np.random.default_rng(3)
    frames = [p + rng.normal(0, 0.2, p.shape).astype(np.float32) for _ in range(3)]
    eng = Engine(make_hp(atom_feature_size=F), atoms.shape[1], device=dev, seed=5)
    eng.freeze_weights(True)
    try:
        rp = ForwardReplay(eng, atoms, frames[0])
        old = rp(frames[1]).clone()
        eng.params.load_state_dict(_moved(eng.params.state_dict()))
        with pytest.raises(ValueError, match="ForwardReplay"):
            rp(frames[1])
        rp2 = ForwardReplay(eng, atoms, frames[0])
        at = torch.from_numpy(atoms).to(dev)
        for k in (2, 1, 0):
            ref = eng.forward(frames_to_batch(at, torch.from_numpy(frames[k]).to(dev)[None], 16, device=dev)).clone()
            got = rp2(frames[k]).clone()
            torch.cuda.synchronize()
            assert torch.equal(ref, got), k
            if k == 1:
                assert not torch.equal(got, old)
        fresh = _fresh(eng, True).forward(frames_to_batch(at, torch.from_numpy(frames[0]).to(dev)[None], 16, device=dev))
        assert torch.equal(fresh, got)
    finally:
        _release(eng)


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("F", [64, 256])
def test_train_replay_refuses_after_an_announced_change_until_an_eager_step(gpu_device, F):
    """TrainStepReplay, load_state_dict, step: the recorded forward would multiply with the images of the old weights.  The step
    raises ValueError naming the remedy and touches nothing; one eager Trainer.step rebuilds the images and the replay continues
    the twin's trajectory bit for bit"""
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.replay import TrainStepReplay
    from nmrgnn_amd.train import Trainer
    dev = gpu_device
    gs = _graphs(6)
    ea, eb = Engine(_hp(F), 10, device=dev, seed=93), Engine(_hp(F), 10, device=dev, seed=93)
    ta, tb = Trainer(ea, lr=1e-3), Trainer(eb, lr=1e-3, cache_images=False)
    try:
        raw0, gp0, y0, w0 = gs[0]
        rp = TrainStepReplay(ta, raw0, y0, w0, graph_ptr=gp0)

        def both(g, replayed):
            la = rp.step(g[0], g[2], g[3]).clone() if replayed else _eager(ta, dev, g)
            lb = _eager(tb, dev, g)
            torch.cuda.synchronize()
            assert torch.equal(la, lb) and torch.equal(ea.params.flat, eb.params.flat), (replayed, float(la), float(lb))

        both(gs[0], True)
        sd = _moved(eb.params.state_dict())
        ea.params.load_state_dict(sd)
        eb.params.load_state_dict(sd)
        keep = (ea.params.flat.clone(), ea.adam_m.clone(), ea.adam_t, ta.step_count)
        with pytest.raises(ValueError, match="eager Trainer.step"):
            rp.step(gs[1][0], gs[1][2], gs[1][3])
        torch.cuda.synchronize()
        assert torch.equal(ea.params.flat, keep[0]) and torch.equal(ea.adam_m, keep[1])
        assert (ea.adam_t, ta.step_count) == keep[2:]
        ea.weights_changed()                                    # the other way of announcing one: refused all the same
        with pytest.raises(ValueError, match="new TrainStepReplay"):
            rp.step(gs[1][0], gs[1][2], gs[1][3])
        both(gs[1], False)
        for k in (2, 3, 4):
            both(gs[k], True)
        assert torch.equal(ea.adam_m, eb.adam_m) and torch.equal(ea.adam_v, eb.adam_v)
    finally:
        ta.close()
        tb.close()
        _release(ea, eb)


# ------------------------------------------------------------------------------------------------------------------ 5b
@pytest.mark.parametrize("F", [64, 256])
def test_replay_after_another_engine_and_an_eager_step_that_keeps_fewer_images(gpu_device, F):
    """another engine takes the device's image cache over (ng_weights_frozen drops every registered PackJob), then this engine
    steps eagerly on a 100-atom batch: below 256 rows the default-width GEMMs keep no piece image, so that step re-registers
    only a part of what the recorded 256-atom chain reads, and ng_adam_step rebuilds only what is registered.  The replayed
    steps behind it must still continue the twin's trajectory.  Second round: the same with a replayed step between the
    change of hands and the small eager step (the jobs stay dropped over a replayed step)"""
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.replay import TrainStepReplay
    from nmrgnn_amd.train import Trainer
    dev = gpu_device
    gs = _graphs(4)
    ea, eb, other = (Engine(_hp(F), 10, device=dev, seed=s) for s in (94, 94, 95))
    ta, tb, to = Trainer(ea, lr=2e-3), Trainer(eb, lr=2e-3, cache_images=False), Trainer(other, lr=2e-3)
    small = _batch(dev, 1, 100, seed=12)
    try:
        raw0, gp0, y0, w0 = gs[0]
        rp = TrainStepReplay(ta, raw0, y0, w0, graph_ptr=gp0)

        def both(la, lb, what):
            torch.cuda.synchronize()
            assert torch.equal(la, lb) and torch.equal(ea.params.flat, eb.params.flat), (what, float(la), float(lb))

        both(rp.step(gs[0][0], gs[0][2], gs[0][3]).clone(), _eager(tb, dev, gs[0]), "replay 0")
        for rnd in (1, 2):
            _eager(to, dev, gs[rnd])
            if rnd == 2:
                # the change of hands happens in front of a REPLAYED step this time: an eager forward of this engine (no weight
                # change) takes the cache back, and the replay behind it registers no image for a rebuild
                ea.forward(small[0])
                both(rp.step(gs[0][0], gs[0][2], gs[0][3]).clone(), _eager(tb, dev, gs[0]), "replay 2, behind the change of hands")
            both(ta.step(*small).clone(), tb.step(*small).clone(), f"small eager step {rnd}")
            both(rp.step(gs[rnd][0], gs[rnd][2], gs[rnd][3]).clone(), _eager(tb, dev, gs[rnd]), f"replay {rnd}a")
            both(rp.step(gs[rnd + 1][0], gs[rnd + 1][2], gs[rnd + 1][3]).clone(), _eager(tb, dev, gs[rnd + 1]), f"replay {rnd}b")
    finally:
        for t in (ta, tb, to):
            t.close()
        _release(ea, eb, other)


# ------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("seed", wc.SEQUENCE_SEEDS)
@pytest.mark.parametrize("F", [64, 256])
def test_seeded_operation_sequences_follow_the_eager_twin(gpu_device, F, seed):
    """weight_cache_cases.sequence(seed) on an engine with every cache on (Trainer with kept images, a TrainStepReplay of shape A,
    frozen and unfrozen validation forwards on the table path, a second engine sharing the device's context), beside a twin
    that packs per call.  After every operation the parameters are the twin's; every validation forward is that of a fresh
    engine holding the current parameters"""
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.replay import TrainStepReplay
    from nmrgnn_amd.train import Trainer
    dev = gpu_device
    seq = wc.sequence(seed)
    gs = _graphs(8)
    eng, twin, other = (Engine(_hp(F), 10, device=dev, seed=s) for s in (41, 41, 43))
    for e in (eng, twin, other):
        e.edge_table_min_edges = 0        # every batch here takes the device-guarded table of the edge function
    tr, tw, to = Trainer(eng, lr=2e-3), Trainer(twin, lr=2e-3, cache_images=False), Trainer(other, lr=2e-3)
    shape_b = _batch(dev, 3, 100, seed=10)
    val, _, _ = _batch(dev, 4, 64, seed=21)
    try:
        raw0, gp0, y0, w0 = gs[0]
        rp = TrainStepReplay(tr, raw0, y0, w0, graph_ptr=gp0)
        assert torch.equal(eng.params.flat, twin.params.flat)
        loads = 0
        for k, op in enumerate(seq):
            g = gs[k % len(gs)]
            la = lb = None
            if op in ("step_a", "replay"):
                la = rp.step(g[0], g[2], g[3]).clone() if op == "replay" else _eager(tr, dev, g)
                lb = _eager(tw, dev, g)
            elif op == "step_b":
                la, lb = tr.step(*shape_b).clone(), tw.step(*shape_b).clone()
            elif op in ("val_frozen", "val_unfrozen"):
                frozen = op == "val_frozen"
                eng.freeze_weights(frozen)
                got = eng.forward(val).clone()
                ref = _fresh(eng, frozen).forward(val)
                torch.cuda.synchronize()
                assert torch.equal(got, ref), (k, op, seq[:k + 1])
            elif op in ("load_step", "excursion", "return"):
                loads += 1
                sd = twin.params.state_dict()
                sd = _moved(sd, loads) if op == "load_step" else _excursion(sd, op == "return")
                eng.params.load_state_dict(sd)
                twin.params.load_state_dict(sd)
                la, lb = _eager(tr, dev, g), _eager(tw, dev, g)
            else:
                assert op == "other_engine"
                _eager(to, dev, g)
            torch.cuda.synchronize()
            assert la is None or torch.equal(la, lb), (k, op, seq[:k + 1])
            assert torch.equal(eng.params.flat, twin.params.flat), (k, op, seq[:k + 1])
        assert torch.equal(eng.adam_m, twin.adam_m) and torch.equal(eng.adam_v, twin.adam_v)
        assert bool(torch.isfinite(eng.params.flat).all())
    finally:
        for t in (tr, tw, to):
            t.close()
        _release(eng, twin, other)
