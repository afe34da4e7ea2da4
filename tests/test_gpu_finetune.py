"""Fine-tuning through Engine, Trainer, GNNModel.fit and the command line: the truncated backward against
the full one bit for bit, its launches against finetune_ref.launch_plan_ref, the grouped update against the full step, and
the refusals.

Models: atom_feature_size 64 and 32 with mp_layers 3, fc_layers 2, edge_fc_layers 2 (no fused live-edge kernels: the edge
paths the switches select are "slots" and, on padded lists, the host-guarded table "table_host"); and, for the other two
tails of the backward, atom_feature_size 64 with edge_fc_layers 4 ("live", and the device-guarded "table").  Three graphs of
20 to 40 atoms, K = 16, as padded neighbour lists and as CSR lists.  Noise and dropout stay on: two forwards with one seed
draw the same numbers, so the kernels of a truncated backward see the inputs of the full one."""
import functools

import numpy as np
import pytest

import finetune_ref as FR

pytestmark = pytest.mark.gpu

C_ELEM, K = 10, 16
MODELS = {"F64": dict(atom_feature_size=64, mp_layers=3, fc_layers=2, edge_fc_layers=2),
          "F32": dict(atom_feature_size=32, mp_layers=3, fc_layers=2, edge_fc_layers=2),
          "F64e4": dict(atom_feature_size=64, mp_layers=3, fc_layers=2, edge_fc_layers=4)}
# mode -> (list form, engine switches, the edge path the forward must report)
MODES = {"nlist-slots": ("nlist", {}, "slots"),
         "nlist-table": ("nlist", {"edge_table_min_edges": 0}, "table_host"),
         "csr-slots": ("csr", {"edge_table_min_edges": 0}, "slots")}
MODES_E4 = {"nlist-live": ("nlist", {}, "live"),
            "nlist-table": ("nlist", {"edge_table_min_edges": 0}, "table"),
            "csr-table": ("csr", {"edge_table_min_edges": 0}, "table"),
            "nlist-slots": ("nlist", {"use_live_edges": False}, "slots")}
SETS = {"out": ["out"], "fc+out": ["fc", "out"], "mp2": ["mp/2"], "mp1+out": ["mp/1", "out"], "mp0": ["mp/0"],
        "embed": ["embed"], "edge_fc": ["edge_fc"], "fc-one-tensor": ["fc/1/bias"],
        "all": ["out", "fc", "mp/0", "mp/1", "mp/2", "embed", "edge_fc"]}
SEED = 77


def hypers(key):
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    return declare_gnn_space(HyperParameters(**MODELS[key]))


def engine(dev, key, switches=None):
    from nmrgnn_amd.engine import Engine
    eng = Engine(hypers(key), C_ELEM, device=dev, seed=5)
    for k, v in (switches or {}).items():
        setattr(eng, k, v)
    return eng


@functools.lru_cache(maxsize=None)
def graphs():
    from nmrgnn_amd import synth
    rng = np.random.default_rng(11)
    out = []
    for n in (20, 33, 40):
        atoms, nl, d = synth.make_graph(n, K, C_ELEM, 0.1, rng)
        out.append((atoms, nl.astype(np.int32), d, synth.inv_degree(nl)))
    N = sum(g[0].shape[0] for g in out)
    return out, rng.standard_normal(N).astype(np.float32), (rng.random(N) < 0.8).astype(np.float32)


def batch(dev, form):
    import torch
    from nmrgnn_amd.graph import concat_graphs
    gs, y, w = graphs()
    gb = concat_graphs(gs, device=dev)
    if form == "csr":
        gb = gb.to_csr()
    return gb, torch.from_numpy(y).to(dev), torch.from_numpy(w).to(dev)


def names_of(eng, groups):
    from nmrgnn_amd import finetune
    return finetune.resolve(groups, list(eng.params.shapes))


def bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


class Spy:
    """engine.lib with every ng_* call recorded as (name, args)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ng_"):
            return fn

        def call(*a):
            self.calls.append((name, a))
            return fn(*a)
        return call

    def of(self, *names):
        return [a for n, a in self.calls if n in names]


def run_backward(eng, gb, y, w, via, **kw):
    """forward(training, SEED) and backward(**kw); the gradient buffer is NaN beforehand.  Returns {tensor: bits}."""
    eng.params.grad.fill_(float("nan"))
    if via == "loss":
        eng.forward(gb, training=True, seed=SEED, loss=(y, w, 1.0))
        dpred = None
    else:
        peaks = eng.forward(gb, training=True, seed=SEED)
        _, dpred = eng.loss_l2(gb, y, w, peaks)
    path = eng.tape.edge_path
    eng.backward(dpred, **kw)
    return {n: bits(eng.params.g(n)) for n in eng.params.shapes}, path


@functools.lru_cache(maxsize=None)
def full_grads(dev, key, mode, via):
    """the full backward's gradients: computed once per (model, mode, call form) and shared"""
    form, switches, want_path = (MODES_E4 if key == "F64e4" else MODES)[mode]
    eng = engine(dev, key, switches)
    gb, y, w = batch(dev, form)
    grads, path = run_backward(eng, gb, y, w, via)
    assert path == want_path, (path, want_path)
    assert all(not np.isnan(g.view(np.float32)).any() for g in grads.values())
    return grads


CASES = [("F64", m, "dpeaks") for m in MODES] + [("F32", m, "dpeaks") for m in MODES] + [("F64", "nlist-slots", "loss")] \
    + [("F64e4", m, "loss" if m == "nlist-live" else "dpeaks") for m in MODES_E4]


@pytest.mark.parametrize("tset", list(SETS))
@pytest.mark.parametrize("key,mode,via", CASES)
def test_truncated_backward(gpu_device, key, mode, via, tset):
    """the gradients of the computed groups are the full backward's bits, the others are never written, and the launches
    are those of the plan"""
    from nmrgnn_amd import finetune
    form, switches, _ = (MODES_E4 if key == "F64e4" else MODES)[mode]
    want = full_grads(gpu_device, key, mode, via)
    eng = engine(gpu_device, key, switches)
    L = eng.L
    gb, y, w = batch(gpu_device, form)
    trainable = names_of(eng, SETS[tset])
    groups = set(finetune.group_names(trainable))
    ref = FR.launch_plan_ref(L, groups)
    csc_calls, fired = [], []
    orig_csc = gb.csc
    gb.csc = lambda: (csc_calls.append(1), orig_csc())[1]
    spy = eng.lib = Spy(eng.lib)
    try:
        got, _ = run_backward(eng, gb, y, w, via, trainable=set(trainable), on_node_grads=lambda: fired.append(len(spy.calls)))
    finally:
        eng.lib = spy._lib
    computed = groups | {"out"}
    for n in eng.params.shapes:
        if finetune.group_of(n) in computed:
            assert np.array_equal(got[n], want[n]), f"{n}: differs from the full backward"
        else:
            assert np.isnan(got[n].view(np.float32)).all(), f"{n}: written although its group is not computed"
    assert sorted(finetune.computed_groups(L, finetune.launch_plan(L, groups))) == sorted(computed)
    # launches
    assert len(spy.of("ng_head_bwd", "ng_head_loss_reduce")) == 1
    fc = spy.of("ng_fc_block_bwd")
    assert len(fc) == (1 if ref["fc_run"] else 0)
    if fc:
        assert (fc[0][-3] is not None) == (fc[0][-2] is not None) == ref["fc_dw"]
    mp = [(n, a) for n, a in spy.calls if n in ("ng_mp_layer_bwd_rec", "ng_mp_layer_bwd_csr")]
    assert len(mp) == len(ref["mp_run"])
    for (n, a), l in zip(mp, ref["mp_run"]):
        dw = a[-1] if n.endswith("csr") else a[-2]
        assert (dw is not None) == (l in ref["mp_dw"]), f"layer {l}"
        if dw is not None:
            assert dw.value == eng.params.g(f"mp/{l}/w").data_ptr()
    assert len(csc_calls) == (1 if ref["edges"] else 0)
    assert len(spy.of("ng_mp_edge_records")) == (1 if ref["edges"] and form == "nlist" else 0)
    assert len(spy.of("ng_embed_bwd")) == (1 if ref["embed"] else 0)
    edge = spy.of("ng_edge_mlp_bwd", "ng_edge_mlp_bwd_tape", "ng_edge_mlp_bwd_live", "ng_edge_table_scatter")
    assert bool(edge) == ref["edge_fc"]
    # the callback: once, behind the flush, which is behind every node-side launch
    assert len(fired) == 1 and len(spy.of("ng_flush_reductions")) == 1
    order = [n for n, _ in spy.calls]
    flush = order.index("ng_flush_reductions")
    assert fired[0] == flush + 1
    node_side = {"ng_head_bwd", "ng_head_loss_reduce", "ng_fc_block_bwd", "ng_mp_layer_bwd_rec", "ng_mp_layer_bwd_csr",
                 "ng_embed_bwd", "ng_mp_edge_records"}
    assert all(i < flush for i, n in enumerate(order) if n in node_side)
    assert eng.tape is None


def snapshot(eng):
    return {"p": eng.params.flat.clone(), "m": eng.adam_m.clone(), "v": eng.adam_v.clone()}


def tensor_bits(eng, buf, name):
    o = eng.params.offsets[name]
    return bits(buf[o:o + int(np.prod(eng.params.shapes[name]))])


# every set on the first model; the sets that end the walk at different stages on the other model, list form and edge MLP
TRAINER_CASES = [("F64", "nlist", t) for t in SETS] + \
    [(k, f, t) for k, f in (("F32", "nlist"), ("F64", "csr"), ("F64e4", "nlist")) for t in ("out", "mp1+out", "edge_fc", "all")]


@pytest.mark.parametrize("key,form,tset", TRAINER_CASES)
def test_trainer_step(gpu_device, key, form, tset):
    """one step: frozen tensors and their moments keep their bits, trainable ones are those of a full step from the same
    state; after three steps the frozen ones are still untouched and the loss is finite"""
    import torch
    from nmrgnn_amd.train import Trainer
    gb, y, w = batch(gpu_device, form)
    a, b = engine(gpu_device, key), engine(gpu_device, key)
    ta, tb = Trainer(a, lr=1e-3, trainable=SETS[tset]), Trainer(b, lr=1e-3)
    try:
        assert ta.trainable == frozenset(names_of(a, SETS[tset]))
        start = snapshot(a)
        la = ta.step(gb, y, w, seed=SEED)
        lb = tb.step(gb, y, w, seed=SEED)
        assert torch.equal(la, lb) and a.adam_t == b.adam_t == 1
        for n in a.params.shapes:
            for buf_a, buf_b, s in ((a.params.flat, b.params.flat, start["p"]), (a.adam_m, b.adam_m, start["m"]),
                                    (a.adam_v, b.adam_v, start["v"])):
                if n in ta.trainable:
                    assert np.array_equal(tensor_bits(a, buf_a, n), tensor_bits(b, buf_b, n)), f"{n}: not the full step's bits"
                else:
                    assert np.array_equal(tensor_bits(a, buf_a, n), tensor_bits(a, s, n)), f"{n}: a frozen tensor moved"
        assert any(not np.array_equal(tensor_bits(a, a.params.flat, n), tensor_bits(a, start["p"], n)) for n in ta.trainable)
        assert ta.trainable_count() == sum(int(np.prod(a.params.shapes[n])) for n in ta.trainable)
        for k in range(2):
            loss = ta.step(gb, y, w, seed=SEED + 1 + k)
        assert np.isfinite(float(loss.item())) and a.adam_t == 3
        for n in a.params.shapes:
            if n not in ta.trainable:
                for buf, s in ((a.params.flat, start["p"]), (a.adam_m, start["m"]), (a.adam_v, start["v"])):
                    assert np.array_equal(tensor_bits(a, buf, n), tensor_bits(a, s, n)), f"{n}: moved within three steps"
        assert torch.isfinite(a.params.flat).all()
        # the forward still runs on current images: the peaks of a second engine loaded with these weights, bit for bit
        c = engine(gpu_device, key)
        c.params.load_state_dict(a.params.state_dict())
        assert torch.equal(a.forward(gb), c.forward(gb))
    finally:
        ta.close()
        tb.close()


def test_trainer_lr_scale_and_clipnorm(gpu_device):
    """lr_scale: the mp tensors move as a full step at half the rate moves them, the others as the full step; a clipnorm far
    above the norm changes no bit and reports the norm of the gradient; one below it shrinks the step"""
    import torch
    from nmrgnn_amd.train import Trainer
    gb, y, w = batch(gpu_device, "nlist")
    engs = [engine(gpu_device, "F64") for _ in range(5)]
    trs = [Trainer(engs[0], lr=1e-3, lr_scale={"mp/1": 2.0, "mp/*": 0.5}), Trainer(engs[1], lr=1e-3),
           Trainer(engs[2], lr=5e-4), Trainer(engs[3], lr=1e-3, clipnorm=1e9), Trainer(engs[4], lr=1e-3, clipnorm=1e-3)]
    try:
        start = snapshot(engs[4])
        for t in trs:
            t.step(gb, y, w, seed=SEED)
        a, full, half, loose, tight = engs
        for n in a.params.shapes:
            want = half if n in ("mp/0/w", "mp/2/w") else full
            if n == "mp/1/w":
                continue
            assert np.array_equal(tensor_bits(a, a.params.flat, n), tensor_bits(want, want.params.flat, n)), n
        assert not np.array_equal(tensor_bits(a, a.params.flat, "mp/1/w"), tensor_bits(full, full.params.flat, "mp/1/w"))
        assert torch.equal(loose.params.flat, full.params.flat) and torch.equal(loose.adam_v, full.adam_v)
        g = full.params.grad.double()
        norm = float(torch.sqrt(sum((full.params.g(n).double() ** 2).sum() for n in full.params.shapes)).item())
        assert g.numel() and norm > 1e-3
        assert trs[3].last_grad_norm() == pytest.approx(norm, rel=1e-12)
        assert trs[4].last_grad_norm() == trs[3].last_grad_norm()
        # clipped to 1e-3: the second moment is that of a gradient (1e-3 / norm) times as large
        k = 1e-3 / norm
        o = tight.params.offsets["out/kernel"]
        v_t, v_f = tight.adam_v[o:o + 8].double().cpu().numpy(), full.adam_v[o:o + 8].double().cpu().numpy()
        assert np.allclose(v_t, v_f * k * k, rtol=1e-5, atol=0)
        assert torch.isfinite(tight.params.flat).all() and not torch.equal(tight.params.flat, start["p"])
        with pytest.raises(ValueError, match="without clipnorm"):
            trs[1].last_grad_norm()
    finally:
        for t in trs:
            t.close()


def test_fit_trainable(gpu_device):
    """fit(trainable=['out/*']) on a two-record set: only the head moves"""
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.hypers import HyperParameters
    from nmrgnn_amd.model import build_GNNModel
    gs, y, w = graphs()
    recs, o = [], 0
    for g in gs[:2]:
        n = g[0].shape[0]
        y_true = np.stack([y[o:o + n], np.zeros(n), np.ones(n)], axis=1).astype(np.float32)
        recs.append(((g[0], g[1], g[2], g[3]), y_true, np.ones(n, np.float32)))
        o += n
    data = ShiftDataset.from_records(recs, device=gpu_device)
    model = build_GNNModel(HyperParameters(**MODELS["F64"]), device=gpu_device)
    assert model.trainable_names(["out/*"]) == ["out/kernel", "out/bias"]
    with pytest.raises(ValueError, match="matches no parameter"):
        model.trainable_names("out/*,head/*")
    model.build(C_ELEM)
    before = model.get_weights()
    hist = model.fit(data, epochs=2, batch_graphs=1, verbose=0, trainable=["out/*"])
    after = model.get_weights()
    assert model.engine.adam_t == 4 and all(np.isfinite(x) for x in hist.history["loss"])
    for n in before:
        assert np.array_equal(before[n], after[n]) == (not n.startswith("out/")), n
    with pytest.raises(ValueError, match="matches no parameter"):
        model.fit(data, epochs=1, verbose=0, trainable=["nothing/*"])


def test_train_command_freeze(gpu_device, tmp_path):
    """train --load --freeze: the saved model's frozen tensors are the checkpoint's, the others moved"""
    from click.testing import CliRunner
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.library import load_model
    from nmrgnn_amd.main import main
    from nmrgnn_amd.model import build_GNNModel
    gs, y, w = graphs()
    recs, o = [], 0
    for g in gs:
        n = g[0].shape[0]
        recs.append(((g[0], g[1], g[2], g[3]), np.stack([y[o:o + n], np.zeros(n), np.ones(n)], axis=1).astype(np.float32),
                     np.ones(n, np.float32)))
        o += n
    rec_file, name, ckpt = str(tmp_path / "a.npz"), str(tmp_path / "model"), str(tmp_path / "ckpt")
    ShiftDataset.from_records(recs, device="cpu").save(rec_file)
    m0 = build_GNNModel(device=gpu_device)
    m0.build(C_ELEM)
    m0.save(ckpt)
    start = m0.get_weights()
    frozen = "embed/*,edge_fc/*,mp/0/*,mp/1/*"
    args = ["train", rec_file, name, "1", "--validation", "0", "--checkpoint-path", ckpt, "--device", str(gpu_device), "--load"]
    res = CliRunner().invoke(main, args + ["--freeze", frozen, "--lr-scale", "mp/*=0.1", "--clipnorm", "1.0"])
    assert res.exit_code == 0, res.output + repr(res.exception)
    n_all = sum(v.size for v in start.values())
    is_frozen = lambda n: n.startswith(("embed/", "edge_fc/", "mp/0/", "mp/1/"))
    n_train = sum(v.size for n, v in start.items() if not is_frozen(n))
    assert f"Training {n_train} of {n_all} parameters: mp/2/w, mp/3/w, fc/0/kernel" in res.output
    end = load_model(name, device=gpu_device).get_weights()
    for n in start:
        assert np.array_equal(start[n], end[n]) == is_frozen(n), n
    for bad in (["--freeze", "embed/*,nope/*"], ["--lr-scale", "zz/*=0.1"], ["--lr-scale", "mp/*"], ["--freeze", "*"],
                ["--clipnorm", "0"]):
        res = CliRunner().invoke(main, args + bad)
        assert res.exit_code == 2, (bad, res.output)


def test_refusals(gpu_device):
    import torch
    eng = engine(gpu_device, "F64")
    gb, y, w = batch(gpu_device, "nlist")
    peaks = eng.forward(gb, training=True, seed=SEED)
    _, dpred = eng.loss_l2(gb, y, w, peaks)
    eg = torch.empty_like(gb.edges)
    with pytest.raises(ValueError, match="full de"):
        eng.backward(dpred, edge_grad=eg, trainable={"out/kernel"})
    with pytest.raises(ValueError, match="full de"):
        eng.backward(dpred, edge_grad=eg, trainable={"mp/1/w"})
    with pytest.raises(ValueError, match="param_grad=False"):
        eng.backward(dpred, edge_grad=eg, param_grad=False, trainable={"out/kernel"})
    for bad in ({"out"}, {"out/kernel", "mp/3/w"}, {"fc/*"}):
        with pytest.raises(ValueError, match="unknown parameter"):
            eng.backward(dpred, trainable=bad)
    assert eng.tape is not None                     # a refused call leaves the tape
    # a set that walks down to layer 0 has the full de: edge_grad is that of the full backward
    eng.backward(dpred, edge_grad=eg, trainable={"embed/kernel"})
    peaks = eng.forward(gb, training=True, seed=SEED)
    eg_full = torch.empty_like(gb.edges)
    eng.backward(dpred, edge_grad=eg_full)
    assert torch.equal(eg.view(torch.int32), eg_full.view(torch.int32))
    with pytest.raises(ValueError, match="unknown parameter"):
        eng.adam_step(groups={"out": 1.0})
    with pytest.raises(ValueError, match="finite"):
        eng.adam_step(groups={"out/kernel": -1.0})
    with pytest.raises(ValueError, match="clipnorm"):
        eng.adam_step(clipnorm=0.0)
    assert eng.adam_t == 0


@pytest.mark.parametrize("form", ["nlist", "csr"])
def test_default_arguments_are_the_old_call(gpu_device, form):
    """backward(trainable=None) and adam_step() without groups against a second engine driven through the argument list
    the package had before fine-tuning: the same bits in the gradients, the weights and both moments"""
    import torch
    gb, y, w = batch(gpu_device, form)
    new, old = engine(gpu_device, "F64"), engine(gpu_device, "F64")
    fired = []
    for step in range(2):
        for eng in (new, old):
            peaks = eng.forward(gb, training=True, seed=SEED + step)
            _, dpred = eng.loss_l2(gb, y, w, peaks)
            if eng is new:
                eng.backward(dpred, on_node_grads=lambda: fired.append(1), edge_grad=None, param_grad=True, trainable=None)
                eng.adam_step(lr=1e-3, grad_scale=0.5, groups=None, clipnorm=None)
            else:
                eng.backward(dpred, lambda: fired.append(1), None, True)
                eng.adam_step(1e-3, 0.5, 0.9, 0.999, 1e-7)
        for x, z in ((new.params.grad, old.params.grad), (new.params.flat, old.params.flat), (new.adam_m, old.adam_m),
                     (new.adam_v, old.adam_v)):
            assert torch.equal(x.view(torch.int32), z.view(torch.int32))
    assert len(fired) == 4 and new.adam_t == old.adam_t == 2
    spy = new.lib = Spy(new.lib)
    try:
        new.forward(gb, training=True, seed=SEED)
        new.backward(dpred)
        new.adam_step()
    finally:
        new.lib = spy._lib
    assert len(spy.of("ng_adam_step")) == 1 and not spy.of("ng_adam_step_groups", "ng_grad_clip_factor")
