"""ng_frames_decode (csrc/traj.hip) through the C ABI against a NumPy decode of the same bytes (tests/traj_ref.py), compared
as integer views, bit for bit: planar and interleaved layouts, both byte orders, atom counts around the 64-lane wave and the
256-atom tile, selections, the count of non-finite values, and every refusal of the entry."""
import numpy as np
import pytest
import torch

from nmrgnn_amd import _lib
from traj_ref import decode_ref

pytestmark = pytest.mark.gpu
assert "ng_frames_decode" in _lib.SIGNATURES       # the binding this file tests

NAN_A, NAN_B, INF_P, INF_M = 0x7fc00001, 0xffabcdef, 0x7f800000, 0xff800000
SENTINEL = 0x12345678


def _dev():
    return torch.device("cuda", 0)


def _layout(kind, n_src, base, gap):
    """(frame_stride, off, elem_stride) of a frame with `base` bytes in front of its data and `gap` bytes behind"""
    if kind == "planar":            # three Fortran records, each between two 4-byte markers
        rec = 4 * n_src + 8
        return base + 3 * rec + gap, (base + 4, base + rec + 4, base + 2 * rec + 4), 4
    return base + 12 * n_src + gap, (base, base + 4, base + 8), 12


def _finite_words(rng, shape):
    w = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    w[(w & 0x7f800000) == 0x7f800000] &= np.uint32(0xbfffffff)      # no word with an all-ones exponent
    return w


def _raw(words, fs, off, es, swap, raw_bytes=None):
    """the chunk holding `words` uint32 [G, n_src, 3] by the layout; every other word is a NaN or Inf bit pattern"""
    G, n_src, _ = words.shape
    nbytes = G * fs if raw_bytes is None else raw_bytes
    order = ">u4" if swap else "<u4"
    fill = np.resize(np.array([NAN_A, INF_P, NAN_B, INF_M], np.uint32), nbytes // 4).astype(order)
    raw = fill.view(np.uint8).copy()
    g, a, c = np.meshgrid(np.arange(G), np.arange(n_src), np.arange(3), indexing="ij")
    at = (g * fs + np.asarray(off)[c] + a * es).reshape(-1)
    raw[at[:, None] + np.arange(4)[None, :]] = words.reshape(-1).astype(order).view(np.uint8).reshape(-1, 4)
    return raw


def _call(raw, G, fs, off, es, swap, n_src, sel, n_out, raw_bytes=None, null=(), ctx_null=False):
    """(rc, out uint32 [G, n_out, 3] on the host, bad) of one ng_frames_decode call; out starts as SENTINEL, bad as 0"""
    dev = _dev()
    ctx = _lib.get_context(0)
    raw_t = torch.from_numpy(raw).to(dev)
    out = torch.full((max(G, 0) * max(n_out, 0) * 3 + 8,), SENTINEL, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    sel_t = None if sel is None else torch.from_numpy(np.asarray(sel, np.int32)).to(dev)
    st = _lib._vp(torch.cuda.current_stream(dev).cuda_stream)
    rc = ctx.lib.ng_frames_decode(None if ctx_null else ctx.handle, st, None if "raw" in null else _lib.ptr(raw_t),
                                  len(raw) if raw_bytes is None else raw_bytes, G, fs, off[0], off[1], off[2], es, swap, n_src,
                                  _lib.ptr(sel_t), n_out, None if "out" in null else _lib.ptr(out),
                                  None if "bad" in null else _lib.ptr(bad))
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[-8:] == SENTINEL).all()         # nothing behind the last row
    return rc, got[:-8], int(bad.cpu()[0])


def _check(words, kind, swap, sel=None, base=0, gap=0):
    G, n_src, _ = words.shape
    fs, off, es = _layout(kind, n_src, base, gap)
    raw = _raw(words, fs, off, es, swap)
    ref, ref_bad = decode_ref(raw, G, fs, off, es, swap, n_src, sel)
    np.testing.assert_array_equal(ref, words if sel is None else words[:, np.asarray(sel)])     # the reference itself
    n_out = n_src if sel is None else len(sel)
    rc, got, bad = _call(raw, G, fs, off, es, swap, n_src, sel, n_out)
    assert rc == 0
    np.testing.assert_array_equal(got.reshape(G, n_out, 3), ref)
    assert bad == ref_bad
    return bad


@pytest.mark.parametrize("kind", ["planar", "interleaved"])
@pytest.mark.parametrize("swap", [0, 1])
def test_layouts_and_sizes(kind, swap):
    rng = np.random.default_rng(11 + swap)
    for n_src in (1, 63, 64, 65, 257, 513):
        for G in (1, 2, 33):
            words = _finite_words(rng, (G, n_src, 3))
            assert _check(words, kind, swap) == 0
            # nonzero offsets, and a frame stride beyond the frame's span: the gap holds NaN and Inf patterns only
            assert _check(words, kind, swap, base=56, gap=4 * n_src + 8) == 0


@pytest.mark.parametrize("kind", ["planar", "interleaved"])
@pytest.mark.parametrize("swap", [0, 1])
def test_selection(kind, swap):
    rng = np.random.default_rng(5)
    n_src, G = 65, 3
    words = _finite_words(rng, (G, n_src, 3))
    perm = rng.permutation(n_src)
    for sel in (None, perm, perm[:17], np.array([64, 0, 64, 64, 3, 0]), np.array([64]), np.array([0]),
                rng.integers(0, n_src, size=300)):         # more outputs than sources: two tiles of one frame
        assert _check(words, kind, swap, sel=sel, base=8, gap=12) == 0


@pytest.mark.parametrize("kind", ["planar", "interleaved"])
@pytest.mark.parametrize("swap", [0, 1])
def test_bits_survive(kind, swap):
    rng = np.random.default_rng(7)
    words = _finite_words(rng, (2, 70, 3))
    special = [0x80000000, 0x00000000, 0x00000001, 0x807fffff, 0x007fffff, NAN_A, NAN_B, 0x7f800001, INF_P, INF_M, 0x7f7fffff]
    words[0, :len(special), 1] = special
    words[1, 69, 2] = NAN_B
    # the five NaNs and Infs of frame 0 and the one of frame 1 arrive as they are and are counted
    assert _check(words, kind, swap) == 6
    assert _check(words, kind, swap, sel=np.array([5, 5, 0, 69])) == 3        # atom 5 of frame 0 twice, atom 69 of frame 1


@pytest.mark.parametrize("kind", ["planar", "interleaved"])
@pytest.mark.parametrize("k", [0, 1, 7])
def test_bad_counter_is_exact(kind, k):
    rng = np.random.default_rng(3 + k)
    G, n_src, n_out = 33, 257, 300
    perm = rng.permutation(n_src)
    sel = np.concatenate([perm[:250], perm[:49], perm[250:251]])            # six atoms stay unselected, 49 come twice
    once = [j for j in range(n_out) if (sel == sel[j]).sum() == 1]         # outputs whose source atom is selected once
    j_first, j_tail = once[0], once[-1]
    assert j_tail >= 256                                                    # a lane of the second, partial tile
    spots = [(0, j_first, 0), (G - 1, j_tail, 2), (0, j_tail, 1), (G - 1, j_first, 1), (G // 2, once[7], 0), (G - 1, j_tail, 0),
             (0, once[100], 2)][:k]
    words = _finite_words(rng, (G, n_src, 3))
    for g, j, c in spots:
        words[g, sel[j], c] = [NAN_A, INF_M, NAN_B, INF_P][(g + j + c) % 4]
    unselected = np.setdiff1d(np.arange(n_src), sel)
    words[:, unselected, :] = NAN_A                                         # never read: never counted
    assert len(unselected) > 0
    for swap in (0, 1):
        assert _check(words, kind, swap, sel=sel, base=4, gap=8) == k


def test_refusals_and_no_launch_cases():
    rng = np.random.default_rng(1)
    G, n_src = 2, 65
    words = _finite_words(rng, (G, n_src, 3))
    fs, off, es = _layout("planar", n_src, 56, 0)
    raw = _raw(words, fs, off, es, 0)
    need = (G - 1) * fs + max(off) + (n_src - 1) * es + 4
    ok = dict(raw=raw, G=G, fs=fs, off=off, es=es, swap=0, n_src=n_src, sel=None, n_out=n_src)

    def refused(**change):
        rc, got, bad = _call(**{**ok, **change})
        assert rc == -1, change                                 # NG_ERR_INVALID
        assert (got == SENTINEL).all() and bad == 0, change     # a host check: nothing was launched
        if not change.get("ctx_null"):
            assert b"frames_decode" in _lib.get_context(0).lib.ng_last_error(_lib.get_context(0).handle)

    refused(ctx_null=True)
    refused(null=("raw",))
    refused(null=("out",))
    refused(null=("bad",))
    refused(fs=fs + 2)
    refused(es=es + 2)
    for c in range(3):
        refused(off=tuple(o + (2 if i == c else 0) for i, o in enumerate(off)))
        refused(off=tuple(o + (1 if i == c else 0) for i, o in enumerate(off)))
    refused(G=-1)
    refused(n_src=-1, sel=np.array([0]), n_out=1)
    refused(n_out=-1, sel=np.array([0]))
    refused(raw_bytes=1 << 31)
    refused(raw_bytes=(1 << 40) + 4)
    refused(n_out=n_src - 1)                                    # no sel: the identity needs n_out == n_src
    refused(n_out=n_src + 1)
    refused(raw_bytes=need - 4)                                 # one word short
    refused(G=G + 1)                                            # a frame more than the chunk holds
    refused(n_src=n_src + 2, n_out=n_src + 2)                   # two atoms more: the last word lies behind the chunk
    # exactly enough bytes is enough
    rc, got, bad = _call(**{**ok, "raw_bytes": need})
    assert rc == 0 and bad == 0
    np.testing.assert_array_equal(got.reshape(G, n_src, 3), words)
    # nothing to do: NG_OK without a launch
    rc, got, bad = _call(**{**ok, "G": 0})
    assert rc == 0 and bad == 0 and (got == SENTINEL).all()
    rc, got, bad = _call(**{**ok, "sel": np.array([0]), "n_out": 0})
    assert rc == 0 and bad == 0 and (got == SENTINEL).all()
