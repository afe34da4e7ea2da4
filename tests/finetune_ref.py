"""Host references for fine-tuning (nmrgnn_amd/finetune.py, csrc/optim.hip), written independently of the
package: the parameter layout, the launch plan of a truncated backward derived from what each stage needs, the segment table
as a run-length code of a per-element scale array, the grouped Adam in float64 on top of node_small_ref.adam_ref, and the
clip factor in float64."""
import itertools
import math

import numpy as np

import node_small_ref as R


# ------------------------------------------------------------------------------------------------- layout
def layout(F, E, H, Le, L, Lf, C):
    """[(name, size)] in buffer order, ({name: offset}, numel): tensors start on multiples of four elements"""
    t = []
    for k in range(Le):
        o = H if k < Le - 1 else E
        t += [(f"edge_fc/{k}/kernel", H * o), (f"edge_fc/{k}/bias", o)]
    t += [(f"mp/{l}/w", F * F * E) for l in range(L)]
    for k in range(Lf):
        o = F if k < Lf - 1 else F // 2
        t += [(f"fc/{k}/kernel", F * o), (f"fc/{k}/bias", o)]
    t += [("out/kernel", F // 2 * C), ("out/bias", C), ("embed/kernel", C * F)]
    off, pos = {}, 0
    for name, size in t:
        pos = -(-pos // 4) * 4
        off[name] = pos
        pos += size
    return t, off, -(-pos // 4) * 4


def all_groups(L):
    return ["out", "fc"] + [f"mp/{l}" for l in range(L)] + ["embed", "edge_fc"]


def group_ref(name):
    head = name.split("/")[0]
    return name.rsplit("/", 1)[0] if head == "mp" else head


# ------------------------------------------------------------------------------------------------- launch plan
def launch_plan_ref(L, groups):
    """What a backward must launch so that every group of ``groups`` gets its gradient, from what each stage consumes:
    the head yields dg; the FC block turns dg into dx (and its own dW); MP layer l turns dh_{l+1} into dh_l, adds its share to
    de (and forms its own dW); the embedding consumes dh_0; the edge MLP consumes de, which is complete only once EVERY MP
    layer has run.  Returns dict(fc_run, fc_dw, mp_run: layers in launch order, mp_dw: those with a dW output, embed, edge_fc,
    edges: the incoming lists, the edge records and de are touched)."""
    groups = set(groups)
    # layer l runs when its own dW is wanted, when a lower layer or the embedding needs dh_l, or when de must be complete
    whole = "embed" in groups or "edge_fc" in groups
    mp_run = [l for l in reversed(range(L)) if whole or any(f"mp/{k}" in groups for k in range(l + 1))]
    fc_run = "fc" in groups or bool(mp_run)
    return dict(fc_run=fc_run, fc_dw="fc" in groups, mp_run=mp_run, mp_dw=[l for l in mp_run if f"mp/{l}" in groups],
                embed="embed" in groups, edge_fc="edge_fc" in groups, edges=bool(mp_run))


def subsets(items):
    for r in range(len(items) + 1):
        for c in itertools.combinations(items, r):
            yield set(c)


# ------------------------------------------------------------------------------------------------- segments
def segments_ref(scales, sizes, offsets, numel):
    """[(begin, end, scale)]: the runs of equal non-zero scale of the per-element scale array, where the padding between
    tensors carries 0 and a run also ends where a new tensor begins with another scale"""
    per = np.zeros(numel, np.float64)
    for name, sc in scales.items():
        per[offsets[name]:offsets[name] + sizes[name]] = sc
    out, i = [], 0
    while i < numel:
        if per[i] == 0.0:
            i += 1
            continue
        j = i
        while j < numel and per[j] == per[i]:
            j += 1
        out.append((i, j, float(per[i])))
        i = j
    return out


# ------------------------------------------------------------------------------------------------- grouped Adam
def rate_ref(lr, b1, b2, step, scale):
    """lr_t * scale as one float32 product"""
    lr_t = R.adam_constants(lr, b1, b2, step)[0]
    return float(np.float32(lr_t) * np.float32(scale))


def adam_groups_ref(p, g, m, v, lr, b1, b2, eps, step, gscale, segs):
    """Grouped Adam in float64 on float32 inputs.  ``segs``: [(begin, end, scale)].  Elements of a segment with scale > 0 get
    node_small_ref.adam_ref's m and v and p - rate * m / (sqrt(v) + eps) with rate = rate_ref; every other element keeps its
    input.  The gradient outside such segments is never looked at: it is replaced by 0 before adam_ref sees it.
    Returns (p, m, v, mag, on): mag as adam_ref's with upd scaled to the segment's rate, on the mask of updated elements."""
    p, g, m, v = (np.asarray(x, np.float32) for x in (p, g, m, v))
    n = p.shape[0]
    on = np.zeros(n, bool)
    rate = np.zeros(n, np.float64)
    for b, e, sc in segs:
        if sc > 0:
            on[b:e] = True
            rate[b:e] = rate_ref(lr, b1, b2, step, sc)
    clean = lambda a: np.where(on, a, np.float32(0))
    _, mi, vi, mag = R.adam_ref(clean(p), clean(g), clean(m), clean(v), lr, b1, b2, eps, step, gscale)
    lr_t = R.adam_constants(lr, b1, b2, step)[0]
    den = np.sqrt(vi) + float(np.float32(eps))
    with np.errstate(invalid="ignore", divide="ignore"):
        pn = p.astype(np.float64) - rate * mi / den
    mag = dict(mag)
    mag["upd"] = mag["upd"] * (rate / lr_t)
    p64, m64, v64 = (a.astype(np.float64) for a in (p, m, v))
    return np.where(on, pn, p64), np.where(on, mi, m64), np.where(on, vi, v64), mag, on


# ------------------------------------------------------------------------------------------------- clip factor
def clip_ref(g, gscale, segs, clipnorm):
    """(factor, norm) in float64: norm^2 = the exactly rounded sum (math.fsum) of the squares of float32(g * gscale) over the
    segments with scale > 0; factor = min(1, clipnorm / norm), 1 where the norm is 0 or not finite"""
    g = np.asarray(g, np.float32)
    sq = []
    for b, e, sc in segs:
        if sc > 0:
            gi = (g[b:e] * np.float32(gscale)).astype(np.float64)
            sq.append(gi * gi)
    tot = math.fsum(np.concatenate(sq)) if sq else 0.0
    norm = math.sqrt(tot) if tot == tot and tot >= 0 else float("nan")
    if not math.isfinite(norm) or norm == 0.0:
        return 1.0, norm
    return min(1.0, clipnorm / norm), norm
