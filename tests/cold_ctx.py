"""Cold-context helpers (test infrastructure): run library calls on a context whose scratch is empty and compare them, bit
for bit, with the same calls on the shared context every other test has long warmed up.

The library states bitwise determinism (tests/test_gpu_determinism.py); scratch offsets, num_cu and split counts do not
depend on how a block of scratch came to exist, so ANY difference between a cold and a warm run is a defect."""
import contextlib
import ctypes as C

import numpy as np


def stream_ptr(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def set_state(ctx, dev, span=0):
    """the explicit state both runs of a comparison start from, whatever an earlier test left behind: the graph span of the
    case, deferral off (flushes what may be queued), replay disarmed, the image cache off"""
    lib, h = ctx.lib, ctx.handle
    ctx.check(lib.ng_ctx_set_graph_span(h, int(span)), "ng_ctx_set_graph_span")
    ctx.check(lib.ng_defer_reductions(h, stream_ptr(dev), 0), "ng_defer_reductions")
    ctx.check(lib.ng_replay_arm(h, 0), "ng_replay_arm")
    ctx.check(lib.ng_weights_frozen(h, 0), "ng_weights_frozen")


@contextlib.contextmanager
def cold_context(device_index=0):
    """A fresh _lib.Context installed as THE context of the device: Engine, GraphBatch, geometry, metrics, dataset, report and
    reweight all reach it through _lib.get_context.  On exit — also when the body raised — the device is synchronised, the
    previous context is put back and the fresh one closed: never more than two contexts alive.  An engine or batch built
    inside holds the closed context and must not be used outside."""
    import torch
    from nmrgnn_amd import _lib
    prev = _lib.get_context(device_index)      # (creates the shared one if this is the first use of the device)
    fresh = _lib.Context(device_index)
    _lib._contexts[device_index] = fresh
    try:
        info = fresh.scratch_info()
        assert not any(info.values()), f"a new context is not cold: {info}"
        yield fresh
    finally:
        try:
            torch.cuda.synchronize(device_index)
        finally:
            _lib._contexts[device_index] = prev
            fresh.close()


def to_host(out):
    """device tensors (or lists of them) of a case's result dict as host arrays; None stays None"""
    def one(v):
        if v is None:
            return None
        if isinstance(v, (list, tuple)):
            return [one(x) for x in v]
        return v.detach().cpu().numpy()
    return {k: one(v) for k, v in out.items()}


def warm_reference(fn, dev, span=0):
    """``fn(ctx) -> dict`` on the shared context in the explicit state: run twice, so that the second run is warm even when this
    is the first test of the process, and the two must agree (the determinism every comparison here rests on)"""
    import torch
    from nmrgnn_amd import _lib
    ctx = _lib.get_context(dev.index or 0)
    set_state(ctx, dev, span)
    try:
        first = to_host(fn(ctx))
        before = ctx.scratch_info()
        second = to_host(fn(ctx))
        torch.cuda.synchronize(dev)
        after = ctx.scratch_info()
    finally:
        set_state(ctx, dev, 0)
    assert_same(first, second, "warm context: two runs")
    return second, (before, after)


def flat(out, prefix=""):
    """(name, array) pairs of a result dict, lists expanded, None dropped"""
    items = []
    for k, v in out.items():
        if isinstance(v, (list, tuple)):
            items += [(f"{prefix}{k}[{i}]", a) for i, a in enumerate(v) if a is not None]
        elif v is not None:
            items.append((f"{prefix}{k}", v))
    return items


def same_bits(a, b):
    """equal as 32-bit patterns (NaN payloads and the sign of zero included), as tests/test_gpu_receptive.py compares"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.itemsize == 4:
        return np.array_equal(a.view(np.int32), b.view(np.int32))
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same(got, ref, what):
    g, r = flat(got), flat(ref)
    assert [n for n, _ in g] == [n for n, _ in r], f"{what}: other outputs"
    bad = []
    for (name, a), (_, b) in zip(g, r):
        if not same_bits(a, b):
            a1, b1 = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
            if a1.shape == b1.shape:
                d = np.flatnonzero(a1.view(np.int32) != b1.view(np.int32)) if a1.dtype.itemsize == 4 else np.flatnonzero(a1 != b1)
                bad.append(f"{name}: {len(d)} of {a1.size} differ, first at flat {int(d[0])}: {a1[d[0]]!r} vs {b1[d[0]]!r}")
            else:
                bad.append(f"{name}: shape {a.shape} vs {b.shape}")
    assert not bad, f"{what}: not the bits of the warm context\n" + "\n".join(bad)
