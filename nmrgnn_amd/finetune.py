"""Fine-tuning: which parameter tensors train, what the backward has to launch for them, and the
segment table of the grouped Adam.  Pure host logic on the names, shapes and offsets of ``params.ParamStore``: no torch,
no GPU.  ``Engine.backward(trainable=)`` / ``Engine.adam_step(groups=)`` and the ``Trainer`` are the users."""
from __future__ import annotations

import math
from collections import namedtuple
from fnmatch import fnmatchcase

MAX_SEGMENTS = 64          # NG_ADAM_MAX_SEGMENTS


def group_of(name):
    """the backward stage that forms the gradient of tensor ``name``: out, fc, mp/l, embed or edge_fc"""
    parts = name.split("/")
    return "/".join(parts[:2]) if parts[0] == "mp" else parts[0]


def group_names(names):
    """the groups of ``names`` in first-appearance order"""
    out = []
    for n in names:
        g = group_of(n)
        if g not in out:
            out.append(g)
    return out


def resolve(patterns, names):
    """The tensors of ``names`` (ordered) that ``patterns`` select, in the order of ``names``.  A pattern is a tensor name
    ("fc/0/bias"), a group name ("mp/2", "fc", "edge_fc": every tensor of the group) or an fnmatch pattern over the tensor
    names ("mp/*", "*/bias").  A string is one pattern, or several separated by commas.  A pattern that selects nothing
    raises ValueError."""
    names = list(names)
    if isinstance(patterns, str):
        patterns = patterns.split(",")
    picked = set()
    for pat in patterns:
        pat = str(pat).strip()
        hit = [n for n in names if n == pat or group_of(n) == pat or fnmatchcase(n, pat)]
        if not hit:
            raise ValueError(f"pattern {pat!r} matches no parameter tensor (tensors: {', '.join(names)})")
        picked.update(hit)
    return [n for n in names if n in picked]


def check_names(trainable, names):
    """``trainable`` as a frozenset of tensor names, each of which must be in ``names``"""
    if isinstance(trainable, str):
        trainable = [trainable]
    known = set(names)
    out = frozenset(str(n) for n in trainable)
    bad = sorted(out - known)
    if bad:
        raise ValueError(f"trainable: unknown parameter tensor(s) {bad} (tensors: {', '.join(names)})")
    return out


# What a backward launches for a trainable set.  fc_run: ng_fc_block_bwd runs; fc_dw: with weight-gradient outputs.
# mp_stop: the MP loop runs l = L-1 .. mp_stop (mp_stop == L: it does not run, and then neither the incoming lists, the
# edge records nor de are touched); mp_dw[l]: layer l gets a dW output.  embed / edge_fc: ng_embed_bwd / the edge-MLP (or
# table) backward run.  The head's gradient and its loss reduction always run.
Plan = namedtuple("Plan", "fc_run fc_dw mp_stop mp_dw embed edge_fc")


def launch_plan(L, groups):
    """the Plan of a model with ``L`` MP layers for the set of trainable ``groups``"""
    groups = set(groups)
    known = {"out", "fc", "embed", "edge_fc"} | {f"mp/{l}" for l in range(L)}
    if groups - known:
        raise ValueError(f"unknown parameter group(s) {sorted(groups - known)}")
    mp_dw = tuple(f"mp/{l}" in groups for l in range(L))
    embed, edge_fc = "embed" in groups, "edge_fc" in groups
    if embed or edge_fc:
        mp_stop = 0             # dh down to the embedding, de summed over every layer
    elif any(mp_dw):
        mp_stop = mp_dw.index(True)
    else:
        mp_stop = L
    fc_dw = "fc" in groups
    return Plan(fc_run=fc_dw or mp_stop < L, fc_dw=fc_dw, mp_stop=mp_stop, mp_dw=mp_dw, embed=embed, edge_fc=edge_fc)


def full_plan(L):
    """the Plan of a backward that trains everything"""
    return launch_plan(L, {"out", "fc", "embed", "edge_fc"} | {f"mp/{l}" for l in range(L)})


def computed_groups(L, plan):
    """the groups whose gradients a backward under ``plan`` defines"""
    out = ["out"]
    if plan.fc_dw:
        out.append("fc")
    out += [f"mp/{l}" for l in range(plan.mp_stop, L) if plan.mp_dw[l]]
    if plan.embed:
        out.append("embed")
    if plan.edge_fc:
        out.append("edge_fc")
    return out


def scales(names, trainable=None, lr_scale=None):
    """{tensor: rate scale} of the trainable tensors: 1, or the scale of the first pattern of ``lr_scale`` ({pattern: scale},
    in its order; patterns as ``resolve``) that selects the tensor.  ``trainable`` None: every tensor."""
    names = list(names)
    train = names if trainable is None else [n for n in names if n in set(trainable)]
    rules = []
    for pat, sc in (lr_scale or {}).items():
        sc = float(sc)
        if not (math.isfinite(sc) and sc >= 0.0):
            raise ValueError(f"lr_scale[{pat!r}] = {sc}: a scale is finite and >= 0")
        rules.append((set(resolve([pat], names)), sc))
    out = {}
    for n in train:
        out[n] = next((sc for hit, sc in rules if n in hit), 1.0)
    return out


def segments(groups, sizes, offsets):
    """[(begin, end, scale)] of the grouped Adam for ``groups`` = {tensor: scale}: tensors not listed, or of scale 0, are in
    no segment; tensors that follow one another in the flat buffer WITHOUT a gap and carry the same scale share one.  The
    alignment padding between two tensors is in no segment (it holds zeros that no launch needs to touch).
    ``sizes`` / ``offsets``: {tensor: element count / first element}, in buffer order."""
    unknown = sorted(set(groups) - set(offsets))
    if unknown:
        raise ValueError(f"groups: unknown parameter tensor(s) {unknown}")
    out = []
    for name, begin in offsets.items():
        sc = float(groups.get(name, 0.0))
        if not (math.isfinite(sc) and sc >= 0.0):
            raise ValueError(f"groups[{name!r}] = {sc}: a scale is finite and >= 0")
        if sc == 0.0:
            continue
        end = begin + int(sizes[name])
        if out and out[-1][1] == begin and out[-1][2] == sc:
            out[-1] = (out[-1][0], end, sc)
        else:
            out.append((begin, end, sc))
    if len(out) > MAX_SEGMENTS:
        raise ValueError(f"groups: {len(out)} segments, the grouped Adam takes at most {MAX_SEGMENTS}")
    return out
