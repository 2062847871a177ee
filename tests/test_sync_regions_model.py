"""tests/sync_model.py against the vectors recorded from the reference's own ActiveRegionDetector (tests/golden/sync_regions/, made by
tools/golden/make_sync_regions_golden.py over tools/golden/sync_regions_driver.cpp): the samples' six coordinates, the synchronised
region, _prevActiveRegionEnd and the id map after every updateEndPosition and after clear().  No GPU."""
import os

import pytest

from tests import active_region_cases as R
from tests import anchor_model as A
from tests import sync_cases as K
from tests import sync_model as S


def test_fixture_is_present_and_small():
    items = K.golden()
    assert sorted(it["name"] for it in items) == ["eight_samples", "one_sample", "three_samples", "two_samples"]
    size = sum(os.path.getsize(os.path.join(K.GOLDEN_DIR, f)) for f in os.listdir(K.GOLDEN_DIR))
    assert size < 300 * 1000


@pytest.mark.parametrize("name", ["one_sample", "two_samples", "three_samples", "eight_samples"])
def test_model_equals_the_recording_call_by_call(name):
    item = next(it for it in K.golden() if it["name"] == name)
    r = K.replay(item, check=True)
    assert len(r["regions"]) >= 3  # (no item is empty; what the fixture must hold is counted in test_fixture_coverage)
    # _prevActiveRegionEnd of every region is the end of the one closed before it: what sk_region_alleles derives from the list
    prev = -1
    for g in r["regions"]:
        assert g["prev_end"] == prev
        prev = g["end"]


@pytest.mark.parametrize("name", ["one_sample", "two_samples", "three_samples", "eight_samples"])
def test_recorded_anchors_are_the_finder_models(name):
    """every sample's finder saw the same calls (the driver checks that they agree): one is_anchor array, sk_ref_anchors' for a finder begun
    at the first call's position"""
    item = next(it for it in K.golden() if it["name"] == name)
    steps = [op for op in item["ops"] if op["op"] == "step"]
    win_begin = steps[0]["win_begin"]
    recorded = "".join(op["anchors"] for op in steps)
    want, _ = A.ref_anchors(item["ref"], item["ref_offset"], win_begin + 1, None, win_begin, len(recorded))
    assert [int(c) for c in recorded] == want


def test_fixture_coverage():
    """a quiet fixture cannot pass: what the generator printed, counted again from the files"""
    c = K.coverage()
    assert c["merged_from_two_or_more"] >= 20
    assert c["delayed_by_another_sample"] >= 5
    assert c["own_merges"] >= 1
    assert c["over_250"] >= 3
    assert c["ploidies_differ"] >= 2
    assert c["sample_counts"] == [1, 2, 3, 8]
    assert c["from_zero"] >= 1 and c["inside_segment"] >= 1
    assert c["clear_branches"] == ["kept", "made", "none"]  # closeActiveRegionDetector :419, :426-434, and the region it does not make
    assert c["clear_with_open_region"] >= 1


def test_windows_chain_through_the_state():
    """the two-sample item was recorded in three windows; one window over all of it gives the same regions and the same state"""
    item = next(it for it in K.golden() if it["name"] == "two_samples")
    r = K.replay(item)
    steps = [w for w in r["windows"] if not w["do_clear"]]
    assert len(steps) == 3
    depth = [sum((w["depth"][s] for w in steps), []) for s in range(2)]
    cand = [sum((w["cand"][s] for w in steps), []) for s in range(2)]
    anchor = sum((w["anchor"] for w in steps), [])
    regions, state, _ = S.sync_active_regions(steps[0]["win_begin"], depth, cand, anchor, steps[-1]["marks"], 2)
    assert regions == sum((w["regions"] for w in steps), [])
    assert state == steps[-1]["state_out"]
    # the cuts: one inside the padding behind a region that is made but not closed, one inside a sample's open region
    assert steps[0]["state_out"]["sync_end"] != 0
    assert any(d["num_variants"] > 0 for d in steps[1]["state_out"]["samples"][:2])


def test_assertions():
    """createActiveRegion's (:318) through a step and through clear(), closeActiveRegion's (:206)"""
    with pytest.raises(S.SyncAssertionFailed):
        state = S.initial_state(1)
        state["samples"][0] = dict(R.UNREACHABLE_STATE)
        S.sync_active_regions(50, [[20] * 40], [[0] * 40], [1] * 40, state=state)
    with pytest.raises(S.SyncAssertionFailed):
        state = S.initial_state(1)
        state["samples"][0] = dict(A.initial_state(), is_beginning=0, active_region_start_pos=90, anchor_pos_following_prev_variant=-1, prev_anchor_pos=44, prev_variant_pos=45,
                                   num_variants=2)
        S.sync_active_regions(50, [[]], [[]], [], state=state, do_clear=True, buf_begin=[40], buf_end=[60])
    with pytest.raises(S.SyncAssertionFailed):
        state = dict(S.initial_state(1), sync_begin=30, sync_end=20)
        S.sync_active_regions(50, [[20] * 4], [[0] * 4], [1] * 4, state=state)


# ---- "single sample: the synchronised region is the region" -------------------------------------------------------------------------------------------

# Items of tests/golden/active_region_detect/walk.json whose synchronised regions are NOT the detector's own, with the reason.  Where the
# detector makes its next region before the last one is closed -- the start position 0 that createActiveRegion leaves (:325) blocks the
# close until the sample's next anchor or candidate, and a candidate that follows at once keeps the start at the anchor before it, below
# end - 1 only if that anchor is -- the two merge into one synchronised region.  Neither recorded walk does that.
SINGLE_SAMPLE_DIFFERENCES = {}


@pytest.mark.parametrize("name", ["from_zero", "inside"])
def test_single_sample_against_the_detectors_own_regions(name):
    w = next(w for w in R.golden()["walks"] if w["name"] == name)
    g = R.recorded_walk(w)
    own, own_state = A.active_regions(g["win_begin"], g["depth"], g["is_candidate"], g["is_anchor"])
    assert own == g["regions"]
    regions, state, _ = S.sync_active_regions(g["win_begin"], [g["depth"]], [g["is_candidate"]], g["is_anchor"], do_clear=False)
    got = [(r["begin"], r["end"]) for r in regions]
    # a region the detector made in the window's last calls may still be open
    if state["sync_end"]:
        got.append((state["sync_begin"], state["sync_end"]))
    same = got == [(b, e) for b, e, _ in own]
    assert same == (name not in SINGLE_SAMPLE_DIFFERENCES), (name, got, own)
    assert state["samples"][0] == own_state
    if same:
        # closed later than made: the nine positions of padding, and the sample's own start 0 until its next anchor or candidate
        for r, (_, e, made_at) in zip(regions, own):
            assert r["closed_at"] > made_at and r["closed_at"] >= e + S.MAX_ASSEMBLY_PADDING
            assert r["sample_mask"] == 1 and r["ploidy"] == [2]
