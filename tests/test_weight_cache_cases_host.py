"""Conditions on the inputs of the weight-cache tests (tests/weight_cache_cases.py): no GPU, nothing measured."""
import os
import re

import numpy as np
import pytest

import weight_cache_cases as wc


def test_every_cached_image_call_site_has_a_case():
    """a search of csrc/*.hip for `image_slot(`: 13 calls (and the definition in repack.hip, which is not one).  A site added
    later fails here until a case names it; a case naming a site that is gone fails too"""
    found = wc.sites()
    assert len(found) == 13, sorted(found)
    named = {s for c in wc.CASES for s in c["sites"]}
    assert named == found, (sorted(found - named), sorted(named - found))


def test_case_names_are_unique_and_kinds_are_stated():
    assert len(set(wc.CASE_NAMES)) == len(wc.CASE_NAMES)
    for c in wc.CASES:
        assert bool(c["kinds"]) == bool(c["sites"]), c["name"]
        assert set(c["sources"]) <= {n for n, _ in c["weights"]}, c["name"]
    kinds = {k for c in wc.CASES for k in c["kinds"]}
    gx = {wc.gx_kind(t, n) for t in (0, 1) for n in (2, 4)}
    assert kinds >= {1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16} | gx, sorted(kinds)


def _csrc(name):
    with open(os.path.join(wc.CSRC, name)) as f:
        return f.read()


def test_image_kind_enum_names_exactly_the_kinds_of_the_cases():
    """`enum ImageKind` of ng_common.h and the formulas of its two family functions, read from the text: together they give the
    kinds the cases name, no more and no fewer, and every member of a family is an enumerator too"""
    text = _csrc("ng_common.h")
    body = re.search(r"enum ImageKind : int \{(.*?)\n\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    enum = {name: int(val) for name, val in re.findall(r"(IK_\w+)\s*=\s*(\d+)", body)}
    assert len(set(enum.values())) == len(enum) and len(enum) == len(re.findall(r"IK_\w+", body)), enum
    gg = re.search(r"constexpr ImageKind gg_image_kind\(int mode\) \{ return \(ImageKind\)\(([^;]*)\); \}", text).group(1)
    gx = re.search(r"constexpr ImageKind gx_image_kind\(int trans, int nbw\) \{ return \(ImageKind\)\(([^;]*)\); \}", text).group(1)
    assert re.fullmatch(r"[\d\s+*a-z]+", gg) and re.fullmatch(r"[\d\s+*a-z]+", gx), (gg, gx)
    gg_kinds = {eval(gg, {"__builtins__": {}}, {"mode": m}) for m in (0, 1)}
    gx_kinds = {eval(gx, {"__builtins__": {}}, {"trans": t, "nbw": n}) for t in (0, 1) for n in (2, 4)}
    assert gx_kinds == {wc.gx_kind(t, n) for t in (0, 1) for n in (2, 4)}
    assert len(gg_kinds) == 2 and len(gx_kinds) == 4 and not gg_kinds & gx_kinds
    assert gg_kinds | gx_kinds <= set(enum.values())
    singles = set(enum.values()) - gg_kinds - gx_kinds
    assert singles == {1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14}, sorted(singles)
    assert set(enum.values()) == {k for c in wc.CASES for k in c["kinds"]}, sorted(enum.items(), key=lambda kv: kv[1])


def test_cache_fields_are_used_in_the_cache_module_alone():
    """member uses (`->name`) of the image cache's fields of ng_ctx, in every source and header of csrc/: only ng_common.h (the
    struct) and repack.hip may hold one.  Local variables of the same names (wimg, wver) are no member uses"""
    member = re.compile(r"(?:->|\.)\s*(wimg|wver|wcache|wowner|wjobs_\w*|replay_token)\b")
    names = sorted(n for n in os.listdir(wc.CSRC) if n.endswith((".hip", ".cuh", ".h")))
    assert "repack.hip" in names and "ng_common.h" in names and len(names) > 40
    found = {}
    for name in names:
        hits = [m.group(0) for m in member.finditer(_csrc(name))]
        if hits:
            found[name] = hits
    assert member.search("ctx->wver++") and member.search("c -> wjobs_dirty") and not member.search("const unsigned wver = f(ctx);")
    assert "repack.hip" in found                     # the search finds the uses that are there
    assert set(found) <= {"repack.hip", "ng_common.h"}, {k: v for k, v in found.items() if k != "repack.hip"}
    # and no call site passes a number for a kind: the third argument of image_slot names an enumerator or a family function
    calls = [(name, m.group(1)) for name in names if name not in ("repack.hip", "ng_common.h")
             for m in re.finditer(r"image_slot\(ctx, [^,]+, ([^,]+),", _csrc(name))]
    assert len(calls) == 13
    for name, kind in calls:
        assert re.match(r"(h2 \? )?(IK_\w+|g[gx]_image_kind\()", kind) and not re.search(r"\b\d", kind), (name, kind)


def test_flagged_and_multi_source_cases_run_their_extra_steps():
    flagged = [c for c in wc.CASES if c["flagged"]]
    multi = [c for c in wc.CASES if len(c["sources"]) > 1]
    # PK_MPW_FWD and PK_MPW_BWD (7, 8) and PK_FC (5) are the kinds with a flag word pair
    assert {k for c in flagged for k in c["kinds"]} == {5, 7, 8}
    assert {k for c in multi for k in c["kinds"]} >= {5, 6, 9, 11, 12, 13}
    for c in wc.CASES:
        s = wc.steps_of(c)
        assert (6 in s) == c["flagged"] and (4 in s) == (len(c["sources"]) > 1), c["name"]
        assert {1, 2, 3, 5, 7, 8} <= set(s), c["name"]
        if c["flagged"]:
            name, idx = c["edge"]
            assert name in c["sources"] and all(i < n for i, n in zip(idx, dict(c["weights"])[name])), c["name"]


@pytest.mark.parametrize("name", wc.CASE_NAMES)
def test_layouts_are_aligned_and_blocks_hold_what_they_say(name):
    c = wc.CASES[wc.CASE_NAMES.index(name)]
    total, table = wc.layout(c)
    assert total % 4 == 0
    spans = []
    for n, (off, shape) in table.items():
        assert (off * 4) % 16 == 0, (name, n)
        spans.append((off, off + int(np.prod(shape))))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total
    b = wc.blocks(c)
    ns = len(c["sources"])
    assert wc.sources_in(c, b["all"]) == (ns, ns)
    assert wc.sources_in(c, b["none"]) == (0, 0) and b["none"][1] > 0
    for blk in b.values():
        assert (blk[0] * 4) % 16 == 0 and blk[0] + blk[1] <= total
    if ns > 1:
        whole, touch = wc.sources_in(c, b["some"])
        assert 0 < whole < ns and touch == whole            # some of the sources, and no source cut in two
        whole_r, touch_r = wc.sources_in(c, b["rest"])
        assert whole_r == ns - whole and touch_r == whole_r
        assert b["some"][0] + b["some"][1] == b["rest"][0] and b["rest"][0] + b["rest"][1] == total
    else:
        assert "some" not in b


@pytest.mark.parametrize("seed", wc.SEQUENCE_SEEDS)
def test_sequences_hold_every_operation_and_the_adjacent_runs(seed):
    seq = wc.sequence(seed)
    assert seq == wc.sequence(seed)                         # a function of the seed alone
    assert len(seq) == wc.SEQUENCE_LENGTH
    assert set(seq) == set(wc.OPS)
    # a replayed step directly in front of a frozen validation forward (the table kept over calls must not survive it)
    assert wc.has_run(seq, ("replay", "val_frozen"))
    # out of the piece range, a replayed step, back in, a replayed step (the flag pair must come down under replay)
    assert wc.has_run(seq, ("excursion", "replay", "return", "replay"))
    # and the longer runs that make the two visible: a frozen forward in front of the first (a table is there to go stale),
    # one more replayed step behind the second (a recorded forward that reads the flag pair)
    for motif in wc.MOTIFS:
        assert wc.has_run(seq, motif), motif


def test_sequences_differ():
    seqs = [tuple(wc.sequence(s)) for s in wc.SEQUENCE_SEEDS]
    assert len(set(seqs)) == len(seqs) == 3
