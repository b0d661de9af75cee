"""The pattern-noise cases on the CPU (tests/pnoise_cases.py; the GPU runs them in tests/test_gpu_pnoise.py): the Python definition is
the oracle's fix_pattern_noise on every content case at debug_flags 0 and in every debug view; the oracle and the reference's own code
give the same bytes on every case, the geometry ones included; each wrong form of the definition differs from it on every case that
names it -- in the corrected frame, or in a debug view where it can only show there -- and the two forms that nothing can show are
asserted to change nothing; and the cases reach what they claim: runs of 1 and of the full 50 pixels, even and odd runs, columns left
with exactly 0, 9, 10 and 11 samples in both directions, pixels equal to white, gradients of exactly 500 and 501, negative odd sums in
both divisions, real 32767 and -32768.  Every comparison is equality of bytes.  No GPU."""
import functools

import numpy as np
import pytest

import pnoise_cases as pc

CONTENT, GEOMETRY = pc.content_cases(), pc.geometry_cases()
ALL = CONTENT + GEOMETRY
OBSERVABLE = [w for w in pc.WRONG if w not in pc.UNOBSERVABLE]
by_name = {c["name"]: c for c in ALL}
names = lambda cases: [c["name"] for c in cases]


@functools.lru_cache(maxsize=None)
def definition(name, flags):
    c = by_name[name]
    return pc.fix(c["frame"], c["white"], flags).tobytes()


@functools.lru_cache(maxsize=None)
def stats_of(name):
    c = by_name[name]
    st = pc.new_stats()
    pc.fix(c["frame"], c["white"], 0, None, st)
    return st


def geometry_views(c):
    """one view per direction: the noise of the column pass, the mask of the row pass"""
    return (4, 9)


def test_the_lists_hold_what_the_gpu_is_to_meet():
    assert len(set(by_name)) == len(ALL) == len(by_name)
    for c in CONTENT:
        assert c["w"] <= 160 and c["h"] <= 160 and c["w"] * c["h"] <= 160 * 64, c["name"]
    # every wrong form is named by a case or listed as unobservable with its reason, never both
    named = {t for c in CONTENT for t in c["tells"]}
    assert named == set(OBSERVABLE) and named.isdisjoint(pc.UNOBSERVABLE) and set(pc.UNOBSERVABLE) <= set(pc.WRONG)
    assert all(len(reason) > 20 for reason in pc.UNOBSERVABLE.values())
    # white levels: none is the synthetic frames' 15000; 65535 (above every int16), a negative one, one inside the data
    whites = {c["white"] for c in ALL}
    assert 15000 not in whites and 65535 in whites and 12000 in whites and any(w < 0 for w in whites)
    # half-extents 768, 769, 2048, 2049 (where the launcher changes the column-median kernel) on both sides, and the smallest frames
    sizes = {(c["w"], c["h"]) for c in GEOMETRY}
    assert sizes == set(pc.GEOMETRY_SIZES)
    for half in (768, 769, 2048, 2049):
        assert (2 * half, 24) in sizes and (24, 2 * half) in sizes
    assert {(2, 2), (4, 20), (20, 4)} <= sizes
    # odd half widths below 26, and a flat frame wider than the reach on both sides
    assert {c["w"] // 2 for c in CONTENT if c["name"].startswith("flat_hw")} == {25, 21, 13}
    assert by_name["flat_wide"]["w"] // 2 > 50
    # a batch holds three different frames of the case's size, the case's own first
    for c in ALL:
        batch = pc.batch_of(c)
        assert len(batch) == 3 and batch[0] is c["frame"] and all(f.shape == c["frame"].shape and f.dtype == np.uint16 for f in batch)
        if c["w"] * c["h"] > 4:
            assert len({f.tobytes() for f in batch}) == 3, c["name"]


@pytest.mark.parametrize("name", names(CONTENT))
def test_the_definition_is_the_oracles(oracle, name):
    c = by_name[name]
    for flags in (0,) + pc.VIEWS:
        want = oracle.fix_pattern_noise(c["frame"], c["white"], flags)
        got = np.frombuffer(definition(name, flags), np.uint16).reshape(want.shape)
        assert np.array_equal(got, want), f"{name} flags {flags}: {(got != want).sum()} px differ, the first at {np.argwhere(got != want)[0].tolist()}"
    assert definition(name, 0) != c["frame"].tobytes() or name == "white_edge_65535"


@pytest.mark.parametrize("name", names(ALL))
def test_the_oracle_is_the_references(oracle, reference, name):
    c = by_name[name]
    for flags in (0,) + (geometry_views(c) if c["geometry"] else pc.VIEWS):
        a, b = oracle.fix_pattern_noise(c["frame"], c["white"], flags), reference.fix_pattern_noise(c["frame"], c["white"], flags)
        assert np.array_equal(a, b), f"{name} flags {flags}: {(a != b).sum()} px differ"


def shows(c, wrong):
    """-> the debug_flags at which the wrong form's bytes differ from the definition's: 0 first, the views only where 0 is blind"""
    for flags in (0,) + pc.VIEWS:
        if pc.fix(c["frame"], c["white"], flags, wrong).tobytes() != definition(c["name"], flags):
            return flags
    return None


@pytest.mark.parametrize("wrong", OBSERVABLE)
def test_each_wrong_form_differs_on_every_case_that_names_it(wrong):
    """on every case that names it in the corrected frame or, where that is blind, in a debug view; and in the corrected frame of one case
    at least, which is what MLVFS sees"""
    naming = [c for c in CONTENT if wrong in c["tells"]]
    assert naming
    where = {c["name"]: shows(c, wrong) for c in naming}
    assert all(f is not None for f in where.values()), (wrong, where)
    assert any(f == 0 for f in where.values()), (wrong, "shows in no corrected frame", where)


@pytest.mark.parametrize("wrong", sorted(pc.UNOBSERVABLE))
def test_the_unobservable_forms_change_nothing(wrong):
    """no_wrap_sum: the smoothed planes are int16 in every view and the noise wraps orig - smoothed again, so both see the sum modulo 2^16.
    clamp1_32768: a column offset is a negated int16 median, so the offsets' median is >= -32767, and -32767 - mc and -32768 - mc are both
    <= 0: the final clamp makes both 0."""
    for c in CONTENT:
        for flags in (0,) + pc.VIEWS:
            assert pc.fix(c["frame"], c["white"], flags, wrong).tobytes() == definition(c["name"], flags), (wrong, c["name"], flags)
    # the first clamp's lower end is met at all: pixels at -32768 under a non-positive offset
    assert (by_name["extremes"]["frame"].view(np.int16) == -32768).any()


def test_the_cases_reach_what_they_claim():
    st = {c["name"]: stats_of(c["name"]) for c in CONTENT}
    runs = set().union(*(s["runs"] for s in st.values()))
    assert 50 in runs and 1 in runs and max(runs) == 50, "no run of the full length, or none of one pixel"
    assert {r % 2 for r in runs} == {0, 1} and {2, 3, 49} <= runs
    # the flat frame's runs are cut by the reach and the row's ends alone: 25 at the left end, 50 inside, 26 at the right end
    wide = st["flat_wide"]["runs"]
    assert {25, 26, 50} <= wide and min(wide) >= min(25, by_name["flat_wide"]["h"] // 2)
    # the narrow flat frames have one run per row: the row
    for name in ("flat_hw25", "flat_hw21", "flat_hw13"):
        assert by_name[name]["w"] // 2 in st[name]["runs"]
    # columns left with exactly 0, 9, 10 and 11 samples, in the first direction (pass 1) and in the second (pass 2)
    for name, passes in (("mask_counts", (1,)), ("mask_counts_t", (2,))):
        for p in passes:
            assert {0, 9, 10, 11} <= {k for q, k in st[name]["samples"] if q == p}, (name, p, sorted(st[name]["samples"]))
    samples = set().union(*(s["samples"] for s in st.values()))
    assert {(1, 9), (1, 10), (2, 9), (2, 10)} <= samples
    # pixels equal to white, at three white levels
    for name in ("white_edge_12000", "white_edge_neg", "walk_tall"):
        assert st[name]["at_white"] > 0, name
        px = by_name[name]["frame"].view(np.int16).astype(int)
        assert {by_name[name]["white"] - 1, by_name[name]["white"] + 1} <= set(np.unique(px).tolist())
    assert st["white_edge_65535"]["at_white"] == 0                      # 65535 is above every int16: nothing is masked by it
    # gradients of exactly 500 and 501, in both directions' cases
    for name in ("grads", "grads_t"):
        assert {500, 501} <= st[name]["grads"], name
    # green averages stepping by exactly 500 and 501
    f = by_name["steps"]["frame"].view(np.int16).astype(int)
    avg = (f[0::2, 1::2] + f[1::2, 0::2]) // 2
    assert {500, 501} <= set(np.abs(np.diff(avg, axis=1)).reshape(-1).tolist())
    # negative odd sums in both divisions (where C division and a shift differ)
    assert sum(s["neg_odd_avg"] for s in st.values()) > 100 and sum(s["neg_odd_mg"] for s in st.values()) > 100
    # real 32767 and -32768, and values on both sides of 32768 in the walks
    ext = by_name["extremes"]["frame"].view(np.int16)
    assert (ext == 32767).sum() > 40 and (ext == -32768).sum() > 40
    for name in ("walk", "walk_tall"):
        px = by_name[name]["frame"].view(np.int16)
        assert (px < -32000).any() and (px > 32000).any(), name
    full = by_name["fullrange"]["frame"]
    assert full.min() < 64 and full.max() > 65535 - 64 and np.unique(full >> 12).size == 16
    # red and blue more than 32767 from green; g1 and g2 further apart than half the range with their average inside the threshold
    rb = by_name["rb_far"]["frame"].view(np.int16).astype(int)
    assert (np.abs(rb[0::2, 0::2] - (rb[0::2, 1::2] + rb[1::2, 0::2]) // 2) > 32767).any()
    gs = by_name["g_split"]["frame"].view(np.int16).astype(int)
    assert (np.abs(gs[0::2, 1::2] - gs[1::2, 0::2]) > 40000).all() and (np.abs(gs[0::2, 1::2] + gs[1::2, 0::2]) < 1000).all()
    # pixels above 32760 under the final clamp, and small ones that it raises to 0
    cl = by_name["clamps"]
    out = np.frombuffer(definition("clamps", 0), np.uint16)
    assert (cl["frame"].view(np.int16) > 32760).any() and (cl["frame"].view(np.int16) < 0).any() and (out == 32760).any() and (out == 0).any()


@pytest.mark.parametrize("name", [c["name"] for c in GEOMETRY if min(c["w"], c["h"]) == 24])
def test_the_geometry_cases_leave_9_10_and_11_of_a_short_columns_12_samples(oracle, name):
    """by the oracle's mask view of the direction whose columns are the frame's short side"""
    c = by_name[name]
    wide = c["w"] >= c["h"]
    mask = oracle.fix_pattern_noise(c["frame"], c["white"], 8 if wide else 9)
    mask = mask if wide else mask.T
    assert set(np.unique(mask).tolist()) == {0, 1000}
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        left = (mask[dy::2, dx::2] == 0).sum(axis=0)
        assert {9, 10, 11, 12} <= set(left.tolist()), (name, dy, dx)
    px = c["frame"].view(np.int16)
    assert (px >= c["white"]).any() and (px < 0).any() and np.unique(px).size > 1000
