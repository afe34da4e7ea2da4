"""The inputs of the weight-cache tests (test_gpu_weight_images.py, test_gpu_weight_state.py), host side only: the table of
cases per `image_slot(` call site of csrc/, the flat weight layouts with their Adam blocks, and the seeded operation
sequences.  test_weight_cache_cases_host.py asserts the conditions these inputs have to meet.

A site is "<file>#<n>": the n-th `image_slot(` call of csrc/<file> in source order (sites() finds them; the definition in
repack.hip is not a call).  Kinds are the values of the ImageKind passed there; ImageKind and PackKind are those of
csrc/ng_common.h."""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nmrgnn_amd", "csrc")


def sites():
    """{"mp_win.hip#0", ...}: every call of image_slot( in csrc/*.hip"""
    out = set()
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(".hip"):
            continue
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        calls = [m for m in re.finditer(r"image_slot\(", text) if not text[:m.start()].endswith("ImageSlot ")]
        out.update(f"{name}#{k}" for k in range(len(calls)))
    return out


def gx_kind(trans, nbw):
    """gx_image_kind of csrc/ng_common.h"""
    return 3 + 16 * trans + 32 * nbw


# steps of the life cycle (test_gpu_weight_images.py): 1 first / second call, 2 announced overwrite, 3 Adam over every source,
# 4 Adam over some of the sources, 5 Adam over none, 6 the edge of the piece range, 7 another owner, 8 cache off.
# A case runs 1, 2, 3, 5, 7, 8, and 4 when it has more than one source, 6 when it is flagged.
#   call     the consumer (test_gpu_weight_images.CALLS)
#   env      the switches that reach the site
#   shape    of the call
#   weights  [(name, shape)] of the flat layout, in order; `sources`: the names the image is packed from
#   kinds    cache kinds the call keeps;  pack: their PackKind;  registered: a PackJob is kept, so ng_adam_step rebuilds the
#            image (one repack_all record at step 3); otherwise the image is rebuilt at its next use and no record appears
#   names    profile scopes that must appear in the first frozen call;  absent: scopes that must not
#   edge     (weight name, index) of the weight step 6 moves to the edge of the range
#   rest_repacks  repack_all records of step 4's second Adam call (the block without the first source): 1 where one of the
#            case's images has ALL its sources there (kind 13: W1, W2, W3), else 0.  The first call of step 4 (the first source
#            alone) and step 5 (no source) must give none: an image with a source outside the block is left to its next use
def _mp(name, site, call, F, E, K, N, kinds, pack, registered=True, flagged=False, env=None, names=(), absent=(), act=1):
    return dict(name=name, sites=site, call=call, env=env or {}, shape=dict(F=F, E=E, K=K, N=N, act=act),
                weights=[("w", (F, F, E))], sources=["w"], kinds=kinds, pack=pack, registered=registered, flagged=flagged,
                names=set(names), absent=set(absent), edge=("w", (3, 5, 0)))


def _edge(name, site, call, kinds, pack, sources, env=None, names=(), absent=(), E=3, n=600, rest_repacks=0):
    H = 128
    w = []
    for t in range(3):
        w += [(f"W{t}", (H, H)), (f"b{t}", (H,))]
    w += [("W3", (H, E)), ("b3", (E,))]
    return dict(name=name, sites=site, call=call, env=env or {}, shape=dict(n=n, H=H, E=E, Le=4, act=1), weights=w,
                sources=sources, kinds=kinds, pack=pack, registered=True, flagged=False, names=set(names), absent=set(absent),
                edge=None, rest_repacks=rest_repacks)


def _fc(name, site, call, F, L, N, kinds, pack, sources, registered=True, flagged=False, env=None, names=(), absent=(), C=0):
    w = []
    for t in range(L):
        w += [(f"W{t}", (F, F if t < L - 1 else F // 2)), (f"b{t}", (F if t < L - 1 else F // 2,))]
    if C:
        w += [("Wout", (F // 2, C)), ("bout", (C,))]
    return dict(name=name, sites=site, call=call, env=env or {}, shape=dict(F=F, L=L, N=N, C=C, act=1), weights=w, sources=sources,
                kinds=kinds, pack=pack, registered=registered, flagged=flagged, names=set(names), absent=set(absent),
                edge=("W1", (7, 9)))


def _dense(name, M, Kin, Nout, cached):
    site = ["gemm_h2.hip#0"] if cached else []
    nbw = lambda n: 4 if n % 256 == 0 else 2
    kinds = (gx_kind(0, nbw(Nout)), gx_kind(1, nbw(Kin))) if cached else ()
    return dict(name=name, sites=site, call="dense", env={}, shape=dict(M=M, Kin=Kin, Nout=Nout, act=1),
                weights=[("W", (Kin, Nout)), ("b", (Nout,))], sources=["W"], kinds=kinds, pack="PK_GX", registered=cached,
                flagged=False, names={"dense_fwd", "dense_dx"} | ({"gemm_range_fallback"} if cached else set()),
                absent=set() if cached else {"gemm_range_fallback", "grad_scale"}, edge=None)


FP32 = {"NG_GEMM_MATH": "fp32"}
GG = {"NG_MP_GG": "1", "NG_MP_GG_MIN_ROWS": "256"}
WIN_NAMES = ("mp_win_fwd", "mp_win_bwd_edge", "mp_win_bwd_node")
# (gemm_range_fallback: the scope of the guarded launch behind every split-operand GEMM — absent where the f32-input GEMM ran)
PLAIN_NAMES = ("mp_aggregate", "mp_update_fwd", "mp_dA", "gemm_range_fallback")

CASES = [
    # ---- F = 64 window kernels: mp_win.hip (forward image 7, strict fp32: 4), mp_win_bwd.hip (8; strict fp32: 14, no job)
    _mp("win_e3_k16", ["mp_win.hip#0", "mp_win_bwd.hip#0"], "mp", 64, 3, 16, 300, (7, 8), "PK_MPW_FWD / PK_MPW_BWD", flagged=True,
        names=WIN_NAMES),
    _mp("win_e1_k8", ["mp_win.hip#0", "mp_win_bwd.hip#0"], "mp", 64, 1, 8, 301, (7, 8), "PK_MPW_FWD / PK_MPW_BWD", flagged=True,
        names=WIN_NAMES),
    _mp("win_w8_e3_k16", ["mp_win.hip#0", "mp_win_bwd.hip#0"], "mp", 64, 3, 16, 300, (7, 8), "PK_MPW_FWD / PK_MPW_BWD",
        flagged=True, env={"NG_MP_W16": "0"}, names=WIN_NAMES),
    _mp("win_fp32_e3_k16", ["mp_win.hip#0", "mp_win_bwd.hip#0"], "mp", 64, 3, 16, 300, (4, 14), "PK_MPW_F32 / none (mpw_pack2)",
        env=FP32, names=WIN_NAMES),      # (the forward image has a job, the backward's has none: one record either way)
    # ---- FC block at F = 64: fc_fused.hip (5), L sources
    _fc("fc_l4", ["fc_fused.hip#0"], "fc", 64, 4, 300, (5,), "PK_FC", ["W0", "W1", "W2", "W3"], flagged=True,
        names=("fc_fused_fwd", "fc_fused_bwd")),
    _fc("fc_l2", ["fc_fused.hip#0"], "fc", 64, 2, 257, (5,), "PK_FC", ["W0", "W1"], flagged=True,
        names=("fc_fused_fwd", "fc_fused_bwd")),
    # ---- edge MLP at H = 128: edge_fwd_h2.hip (6: W0..W3), edge_bwd_h2.hip (13: W1, W2, W3, the row sums behind the fragments)
    _edge("edge_h2_e3", ["edge_fwd_h2.hip#0", "edge_bwd_h2.hip#0"], "edge", (6, 13), "PK_EDGE_H2 / PK_EDGE_WT",
          ["W0", "W1", "W2", "W3"], names=("edge_fwd_h2", "edge_bwd_h2_prep", "edge_bwd_h2"), absent=("edge_fused_fwd",),
          rest_repacks=1),
    _edge("edge_h2_e1", ["edge_fwd_h2.hip#0", "edge_bwd_h2.hip#0"], "edge", (6, 13), "PK_EDGE_H2 / PK_EDGE_WT",
          ["W0", "W1", "W2", "W3"], names=("edge_fwd_h2", "edge_bwd_h2"), absent=("edge_fused_fwd",), E=1, n=601, rest_repacks=1),
    # ---- the f32-input edge kernels: edge_fused.hip (11: W0..W2 forward fragments), edge_fused_bwd.hip (12: transposed)
    _edge("edge_fp32_e3", ["edge_fused.hip#0", "edge_fused_bwd.hip#0"], "edge", (11, 12), "PK_EDGE_F32", ["W0", "W1", "W2"],
          env={"NG_EDGE_MATH": "fp32"}, names=("edge_fused_fwd",), absent=("edge_fwd_h2", "edge_bwd_h2")),
    # ---- molecule-sized inference at F = 256: frame_fused.hip (9: one image per FC weight; 10: the MPLayer weight), no jobs
    _fc("fc_head", ["frame_fused.hip#0"], "fc_head", 256, 4, 300, (9,), "none (ff_pack_kernel)", ["W0", "W1", "W2", "W3"],
        registered=False, names=("fc_head_short",), C=10),
    _mp("mp_short_e3", ["frame_fused.hip#1"], "mp_short", 256, 3, 16, 300, (10,), "none (ff_pack_mp_kernel)", registered=False,
        names=("mp_layer_short",)),
    _mp("mp_short_e1", ["frame_fused.hip#1"], "mp_short", 256, 1, 8, 290, (10,), "none (ff_pack_mp_kernel)", registered=False,
        names=("mp_layer_short",)),
    # ---- the generic MPLayer: node_ops.hip (1: the plain GEMM form), with the piece images gemm_h2_prepack_mp packs from w
    #      itself (gemm_h2.hip#1) that gx_launch then finds valid (gemm_h2.hip#0)
    _mp("mp_plain_256", ["node_ops.hip#0", "gemm_h2.hip#1", "gemm_h2.hip#0"], "mp", 256, 3, 16, 300,
        (1, gx_kind(0, 4), gx_kind(1, 4)), "PK_MP_PLAIN / PK_GX", names=PLAIN_NAMES, absent=("mp_gg_fwd", "mp_win_fwd")),
    _mp("mp_plain_128", ["node_ops.hip#0", "gemm_h2.hip#1", "gemm_h2.hip#0"], "mp", 128, 3, 16, 4100,
        (1, gx_kind(0, 2), gx_kind(1, 2)), "PK_MP_PLAIN / PK_GX", names=PLAIN_NAMES, absent=("mp_gg_fwd", "mp_win_fwd")),
    # ---- gather-GEMM: mp_gg.hip (15 forward, 16 pull)
    _mp("mp_gg", ["mp_gg.hip#0"], "mp", 256, 3, 16, 300, (15, 16), "PK_GG", env=GG, names=("mp_gg_fwd", "mp_gg_pull")),
    # ---- dense GEMMs: gemm_h2.hip#0 with the weight itself as the key, on both sides of gemm_h2_fwd_ok's row thresholds
    #      (256 rows with 256-column tiles, 4096 rows otherwise); below them no image is kept at all
    _dense("dense_255", 255, 256, 256, False),
    _dense("dense_256", 256, 256, 256, True),
    _dense("dense_4095", 4095, 384, 384, False),
    _dense("dense_4096", 4096, 384, 384, True),
]
CASE_NAMES = [c["name"] for c in CASES]


def steps_of(case):
    s = [1, 2, 3]
    if len(case["sources"]) > 1:
        s.append(4)
    s.append(5)
    if case["flagged"]:
        s.append(6)
    return s + [7, 8]


# ------------------------------------------------------------------------------------------------- flat weight layout
PAD_FLOATS = 64      # a block of parameters that feeds no image, in front of and behind the case's weights


def layout(case):
    """offsets (floats) of every weight in ONE flat buffer, as ParamStore lays an engine's out: each at a 16-byte boundary.
    Returns (total floats, {name: (offset, shape)}) with the extra blocks "_head" and "_tail"."""
    off, table = 0, {}
    for name, shape in [("_head", (PAD_FLOATS,))] + list(case["weights"]) + [("_tail", (PAD_FLOATS,))]:
        table[name] = (off, tuple(shape))
        off += (int(np.prod(shape)) + 3) // 4 * 4
    return off, table


def blocks(case):
    """the (offset, count) blocks of ng_adam_step, in floats: "all" holds every source, "some" a proper part of them and
    "rest" the others (multi-source cases), "none" no source"""
    total, table = layout(case)
    size = lambda n: int(np.prod(table[n][1]))
    out = {"all": (0, total), "none": (table["_tail"][0], PAD_FLOATS)}
    if len(case["sources"]) > 1:
        first = case["sources"][0]
        cut = table[first][0] + size(first)
        out["some"] = (0, cut)
        out["rest"] = (cut, total - cut)
    return out


def sources_in(case, block):
    """how many of the case's sources lie wholly inside `block`, and how many touch it"""
    _, table = layout(case)
    lo, hi = block[0], block[0] + block[1]
    whole = touch = 0
    for n in case["sources"]:
        a = table[n][0]
        b = a + int(np.prod(table[n][1]))
        whole += a >= lo and b <= hi
        touch += a < hi and b > lo
    return whole, touch


# ------------------------------------------------------------------------------------------------ operation sequences
OPS = ("step_a", "step_b", "replay", "val_frozen", "val_unfrozen", "load_step", "excursion", "return", "other_engine")
SEQUENCE_SEEDS = (11, 12, 13)
SEQUENCE_LENGTH = 30
# the weights "excursion" takes out of the fp16 piece range (|2^8 w| >= 65504) and "return" sets to 0.25; both are a
# load_state_dict followed by ONE eager step of shape A (what a replayed step needs after an announced change)
EXCURSION = (("mp/1/w", (3, 5, 0), 400.0), ("mp/2/w", (40, 63, 2), -300.0), ("fc/1/kernel", (7, 9), 350.0))
# the runs every sequence holds as adjacent operations.  The first: a frozen validation forward keeps a table, a replayed step
# moves the weights, the next frozen forward must not read it.  The second: out of the range, a replayed step (the recorded
# repack raises the flag pair), back, a replayed step (it must lower it), and one more, whose recorded forward reads the pair
MOTIFS = (("val_frozen", "replay", "val_frozen"), ("excursion", "replay", "return", "replay", "replay"))


def sequence(seed):
    """SEQUENCE_LENGTH operations: every kind at least once, and each of MOTIFS as adjacent operations"""
    rng = np.random.default_rng(seed)
    free = SEQUENCE_LENGTH - sum(len(m) for m in MOTIFS)
    body = list(OPS) + [OPS[int(rng.integers(len(OPS)))] for _ in range(free - len(OPS))]
    order = rng.permutation(len(body))
    parts = [[body[int(i)]] for i in order]
    for m in MOTIFS:
        parts.insert(int(rng.integers(len(parts) + 1)), list(m))
    return [op for p in parts for op in p]


def has_run(seq, motif):
    n = len(motif)
    return any(tuple(seq[i:i + n]) == tuple(motif) for i in range(len(seq) - n + 1))
