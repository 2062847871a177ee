"""Active regions on the device (sk_ref_anchors, sk_active_regions, csrc/active_region_detect.hip): every byte of every output equals
the loop model (tests/anchor_model.py, itself pinned to vectors recorded from the reference by
tests/test_active_region_detect_model.py)."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from strelka_amd import capi
from tests import active_region_cases as R
from tests import anchor_model as A
from tests import intake_cases as K
from tests import intake_model as M

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024        # AR_TILE: positions per workgroup of the tract kernel
HEAD = 210         # AR_HEAD: positions from m answered by the reference's own walk
WALK_CHUNK = 16384  # AR_WALK_CHUNK: positions the walk takes per turn
N_POS_EDGES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4096]


def _anchors(ref, ref_offset, init_pos, init_span, win_begin, n_pos, span_pos=(), what=""):
    """device against model -> (is_anchor list, rows)"""
    capi.init(0)
    want, want_rows = A.ref_anchors(ref, ref_offset, init_pos, init_span, win_begin, n_pos, span_pos)
    got, got_rows = capi.ref_anchors(ref, ref_offset, init_pos, init_span, win_begin, n_pos, span_pos)
    assert got.dtype == np.uint8 and len(got) == n_pos
    bad = [i for i, (a, b) in enumerate(zip(got.tolist(), want)) if a != b]
    assert not bad, "%s: %d / %d anchors differ, first at position %d: device %d, model %d" % (what, len(bad), n_pos, win_begin + bad[0], got[bad[0]], want[bad[0]])
    assert got_rows.tolist() == want_rows, what
    return want, want_rows


def _sites(pairs):
    a = np.zeros(len(pairs), capi.INTAKE_SITE_DTYPE)
    for i, (c, d) in enumerate(pairs):
        a[i] = (c, d)
    return a


def _state_dict(s):
    return {k: int(s[k][0]) for k in capi.AR_STATE_DTYPE.names}


def _walk(win_begin, depth, cand, anchor, state=None, what="", counts=None):
    """device against model -> (regions, state_out) of the model"""
    capi.init(0)
    want_regions, want_state = A.active_regions(win_begin, depth, cand, anchor, state)
    sites = _sites(list(zip(counts or [0] * len(depth), depth)))
    got_regions, got_state = capi.active_regions(win_begin, sites, cand, anchor, None if state is None else capi.ar_state(state))
    assert [tuple(int(x) for x in r) for r in got_regions] == want_regions, what
    assert _state_dict(got_state) == want_state, what
    return want_regions, want_state


# ---- anchors: tracts at the rule's edges --------------------------------------------------------------------------------------------------------------


def _both_paths(ref, what, init_span=None):
    """the tract at R.TRACT_AT = 400 through the tract kernel (a finder begun at the segment's start, m = 0) and through the head kernel
    (a finder begun 100 before the tract)"""
    n = len(ref)
    far = _anchors(ref, 0, 0, init_span, 0, n + 30, what=what + ", far from m")[0]
    near = _anchors(ref, 0, R.TRACT_AT - 1, init_span, R.TRACT_AT - 100, n + 130 - R.TRACT_AT, what=what + ", near m")[0]
    return far, near


@pytest.mark.parametrize("length", [2, 3, 4])
def test_homopolymers_of_2_3_4(length):
    far, near = _both_paths(R.tract_reference(1, length), "homopolymer %d" % length)
    want = [] if length == 2 else list(range(R.TRACT_AT, R.TRACT_AT + length))
    assert [i for i, x in enumerate(far) if not x] == want
    assert [R.TRACT_AT - 100 + i for i, x in enumerate(near) if not x] == want


@pytest.mark.parametrize("u", [1, 2, 3, 49, 50])
def test_tract_of_2u_minus_1_against_2u(u):
    short = 2 if u == 1 else 2 * u - 1
    full = 3 if u == 1 else 2 * u
    far, near = _both_paths(R.tract_reference(u, short), "unit %d, %d bases" % (u, short))
    assert all(far) and all(near)
    far, near = _both_paths(R.tract_reference(u, full), "unit %d, %d bases" % (u, full))
    assert [i for i, x in enumerate(far) if not x] == list(range(R.TRACT_AT, R.TRACT_AT + full))
    _both_paths(R.tract_reference(u, 3 * u + 1), "unit %d, %d bases" % (u, 3 * u + 1))


def test_period_51_is_no_repeat():
    far, near = _both_paths(R.tract_reference(51, 153), "period 51")
    assert all(far) and all(near)


def test_n_inside_a_tract_and_n_as_the_earlier_base():
    at = R.TRACT_AT
    for u, total in ((1, 12), (3, 20), (50, 160)):
        ref = R.tract_reference(u, total)
        plain = _both_paths(ref, "unit %d" % u)[0]
        for k in (0, u, total // 2, total - 1):  # the tract's first base is base(q - u) of its first match
            cut = ref[:at + k] + "N" + ref[at + k + 1:]
            got = _both_paths(cut, "unit %d, N at %d" % (u, k))[0]
            if 0 < k < total - 1 and total // 2 == k:
                assert got != plain
    _both_paths(R.thue(400, "ACG") + "N" * 40 + R.thue(360, "ACG"), "a run of N")  # N == N is no match: every position stays an anchor


@pytest.mark.parametrize("u", [1, 2, 7, 50])
def test_tract_crossing_m(u):
    """m three matches into a tract's run of match_u: span_u(m - 1) is the stale slot's -- zero, 2u - 1 (the trigger 2u falls on m), 2u and more (the
    trigger is stepped over: no back-unset, every position of the run a hit from m on)"""
    total = 3 * u + 9
    ref = R.tract_reference(u, total)
    m = R.TRACT_AT + u + 3
    results = {}
    for name, value in (("zero", 0), ("2u-1", 2 * u - 1), ("2u", 2 * u), ("2u+5", 2 * u + 5), ("u", u)):
        init = [0] * A.MAX_REPEAT_UNIT
        init[u - 1] = value
        results[name] = _anchors(ref, 0, m + 99, init, m, len(ref) - m + 20, [m, m + 1, R.TRACT_AT + total - 1, R.TRACT_AT + total],
                                 what="unit %d, init %s" % (u, name))
    assert results["zero"][1][0][u - 1] == 1 and results["2u-1"][1][0][u - 1] == 2 * u and results["2u+5"][1][0][u - 1] == 2 * u + 6
    _anchors(ref, 0, m + 99, None, m, len(ref) - m + 20, what="unit %d, init NULL" % u)
    rng = np.random.default_rng(700 + u)
    _anchors(ref, 0, m + 99, [int(x) for x in rng.integers(0, 140, A.MAX_REPEAT_UNIT)], m, len(ref) - m + 20, [m], what="unit %d, random init" % u)
    _anchors(ref, 0, m + 99, [0xFFFFFFFF - 2] * A.MAX_REPEAT_UNIT, m, 300, [m, m + 2, m + 3], what="unit %d, init near 2^32" % u)


@functools.lru_cache(maxsize=None)
def _long_reference():
    """3 600 repeat-rich bases at offset 1000, a 600-base homopolymer at 2200 .. 2799 and tracts up to the segment's last base"""
    rng = np.random.default_rng(8101)
    ref = K.repeat_rich_reference(3600, rng)
    ref = ref[:1200] + "A" * 600 + "C" + ref[1801:]
    return ref[:3560] + "TG" * 20, 1000


def test_windows_cut_through_tracts_and_the_segments_end():
    """windows beginning and ending inside the homopolymer, tile edges inside it (the tiles begin at max(win_begin, m + 210)), the
    segment's last bases (a tract up to the end; beyond it get_base gives N), windows wholly past the segment"""
    ref, off = _long_reference()
    end = off + len(ref)
    for win_begin, n_pos in ((2205, 300), (2100, 400), (2300 - TILE, TILE + 50), (2500 - 2 * TILE + 1000, 2 * TILE), (2799, 1), (2800, 1), (2199, 2),
                             (end - 300, 300), (end - 300, 500), (end - 1, 1), (end, 200), (end + 150, 70), (1000, end - 1000 + 130)):
        _anchors(ref, off, 1000, None, win_begin, n_pos, what="window %d + %d" % (win_begin, n_pos))
    _anchors(ref, off, 2500, None, 2401, 900, what="m inside the homopolymer")


def test_segment_start_where_pos_minus_u_is_before_the_segment():
    ref = "CACACACACA" + K.repeat_rich_reference(700, np.random.default_rng(8102))
    for ref_offset, init_pos in ((0, 0), (0, 30), (0, 98), (0, 99), (0, 100), (500, 400), (500, 560), (500, 700)):
        m = A.min_pos(init_pos, ref_offset)
        _anchors(ref, ref_offset, init_pos, None, m, ref_offset + len(ref) - m + 10, [m], what="offset %d, init_pos %d" % (ref_offset, init_pos))


@pytest.mark.parametrize("n_pos", N_POS_EDGES)
def test_window_sizes_at_the_edges(n_pos):
    ref, off = _long_reference()
    m = A.min_pos(1100, off)
    for win_begin in (m, m + 1, m + HEAD - 1, m + HEAD, m + HEAD + 700):  # head only / head and tiles / tiles only
        _anchors(ref, off, 1100, None, win_begin, n_pos, what="win_begin m + %d, n_pos %d" % (win_begin - m, n_pos))


def test_window_in_pieces_equals_the_whole():
    capi.init(0)
    ref, off = _long_reference()
    init = [int(x) for x in np.random.default_rng(8103).integers(0, 110, A.MAX_REPEAT_UNIT)]
    whole, _ = capi.ref_anchors(ref, off, 1050, init, 1000, 3700)
    assert whole.tolist() == A.ref_anchors(ref, off, 1050, init, 1000, 3700)[0]
    for cuts in ((0, 1500, 3700), (0, 100, 1300, 3700), (0, 209, 210, 3700), (0, 1, 2234, 3700)):
        parts = [capi.ref_anchors(ref, off, 1050, init, 1000 + a, b - a)[0] for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate(parts).tobytes() == whole.tobytes(), cuts
    assert len(capi.ref_anchors(ref, off, 1050, init, 1000, 0)[0]) == 0


def test_span_rows():
    ref, off = _long_reference()
    end = off + len(ref)
    _, rows = _anchors(ref, off, 1050, None, 1000, 10, [1000, 1001, 2200, 2500, 2799, 2800, end - 1, end, end + 40], what="span rows")
    assert rows[3][0] == 1 + 300 and rows[4][0] == 600 and rows[5][0] == 1  # inside the homopolymer, at its end, past it
    init = list(range(200, 250))
    _, rows = _anchors(ref, off, 2500, init, 2401, 10, [2401, 2402, 2799, 2800], what="span rows from a stale slot")
    assert rows[0][0] == 201 and rows[2][0] == 200 + 399  # the run reaches back to m: the stale value carries
    _anchors(ref, off, 1050, None, 1000, 0, [1500], what="rows only")


def test_device_entry_takes_an_odd_reference_address_and_flags_a_bad_span_position():
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    ref, off = _long_reference()
    p = lambda t: C.c_void_p(t.data_ptr())
    raw = np.frombuffer(b"G" + ref.encode(), np.uint8).copy()
    d_ref = torch.from_numpy(raw).cuda()[1:]
    assert d_ref.data_ptr() % 2 == 1
    n_pos = 3000
    d_anchor = torch.full((n_pos + 64,), 7, dtype=torch.uint8, device="cuda")
    span_pos = np.array([1000, 999, 2500], np.int32)
    d_span_pos = torch.from_numpy(span_pos).cuda()
    d_rows = torch.full((3, 50), 9, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    capi._check(L.sk_ref_anchors_dev(p(d_ref), off, len(ref), 1050, None, 1000, n_pos, p(d_anchor), 3, p(d_span_pos), p(d_rows), st))
    torch.cuda.synchronize()
    want, want_rows = A.ref_anchors(ref, off, 1050, None, 1000, n_pos, [1000, 2500])
    got = d_anchor.cpu().numpy()
    assert got[:n_pos].tolist() == want and (got[n_pos:] == 7).all()
    rows = d_rows.cpu().numpy().astype(np.uint32)
    assert rows[0].tolist() == want_rows[0] and rows[2].tolist() == want_rows[1] and not rows[1].any()
    assert L.sk_check_device_errors() != 0 and "span_pos" in capi.last_error()
    assert L.sk_check_device_errors() == 0  # (cleared)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------------------------------


def _flags(n, cand=(), zero=(), not_anchor=(), depth=20):
    """n positions, all ring anchors of depth 20 unless listed (window offsets)"""
    c = [0] * n
    d = [depth] * n
    a = [1] * n
    for i in cand:
        c[i] = 1
    for i in zero:
        d[i] = 0
        c[i] = 1  # (count 0 >= 0.35f * 0: the intake flags every depth-zero position whose reference is not N)
    for i in not_anchor:
        a[i] = 0
    return d, c, a


def test_candidates_13_apart_and_14_apart():
    regions, _ = _walk(100, *_flags(80, cand=(20, 33)), what="13 apart")
    assert regions == [(119, 135, 148)]  # both in one region: [anchor before, anchor after + 1), made at the first event more than 13 past 133
    regions, _ = _walk(100, *_flags(80, cand=(20, 34)), what="14 apart")
    assert regions == []
    regions, _ = _walk(100, *_flags(80, cand=(20, 33, 47)), what="three")
    assert regions == [(119, 135, 148)]  # 147 is 14 past 133: the pair is closed when 147 arrives, and 147 starts over alone
    regions, _ = _walk(100, *_flags(80, cand=(20, 33, 46)), what="three, 13 apart")
    assert regions == [(119, 148, 161)]


def test_one_candidate_alone_gives_no_region():
    regions, state = _walk(100, *_flags(60, cand=(20,)), what="alone")
    assert regions == [] and state["num_variants"] == 0


def test_depth_zero_candidates():
    # with no variant counted it is none -- and, being a ring anchor, it is a plain anchor
    regions, _ = _walk(100, *_flags(60, zero=(10, 11, 12)), what="depth zero, nothing open")
    assert regions == []
    # with one counted it counts: 120 and the depth-zero 125 make a region
    regions, _ = _walk(100, *_flags(60, cand=(20,), zero=(25,)), what="depth zero, region open")
    assert regions == [(119, 127, 140)]
    # ... also where it is no ring anchor; and one that is no ring anchor with nothing open is no event at all
    _walk(100, *_flags(60, cand=(20,), zero=(25,), not_anchor=(25, 26, 27)), what="depth zero, no ring anchor")
    _walk(100, *_flags(60, zero=(5, 6), not_anchor=(4, 5, 6, 7)), what="depth zero, no ring anchor, nothing open")
    # a stretch of depth zero after a pair: the first 13 count, the one after closes the region and is a plain anchor again
    regions, _ = _walk(100, *_flags(90, cand=(20, 22), zero=tuple(range(23, 70))), what="depth-zero stretch")
    assert len(regions) == 1


def test_window_from_position_0_where_start_0_reads_as_unset():
    regions, _ = _walk(0, *_flags(60, cand=(1, 3)), what="from 0")
    # position 0 is an anchor and sets the start to 0; at the second candidate the start 0 reads as unset (:400) and becomes the anchor 2
    assert regions == [(2, 5, 18)]
    _walk(0, *_flags(90, cand=(1, 3, 40, 43), not_anchor=(0,)), what="from 0, no anchor at 0")
    _walk(0, *_flags(60, cand=(0, 2)), what="candidate at 0")
    state = dict(A.initial_state(), is_beginning=0, active_region_start_pos=0, anchor_pos_following_prev_variant=3, prev_anchor_pos=7)
    _walk(8, *_flags(60, cand=(2, 4), not_anchor=(0, 1, 2, 3, 4)), state=state, what="start 0 carried in")


def test_open_region_is_carried_to_the_next_window():
    d, c, a = _flags(120, cand=(50, 55), not_anchor=tuple(range(56, 60)))
    whole, _ = _walk(100, d, c, a, what="whole")
    assert whole == [(149, 161, 170)]
    first, state = _walk(100, d[:58], c[:58], a[:58], what="first part")  # no anchor after the last variant yet
    assert first == [] and state["num_variants"] == 2 and state["anchor_pos_following_prev_variant"] == -1
    second, _ = _walk(158, d[58:], c[58:], a[58:], state=state, what="second part")
    assert second == whole


def test_no_anchor_for_more_than_13_positions():
    d, c, a = _flags(120, cand=(30, 33), not_anchor=tuple(range(34, 60)))
    regions, _ = _walk(100, d, c, a, what="no anchor for 26")
    assert regions == [(129, 161, 162)]  # the first anchor, 160, follows the variants; the event after it closes the region
    _walk(100, *_flags(120, cand=(30, 33, 70), not_anchor=tuple(range(34, 80))), what="a candidate before any anchor")
    _walk(100, *_flags(120, cand=(30, 33), not_anchor=tuple(range(0, 30)) + tuple(range(34, 120))), what="no anchor at all")


def test_candidate_on_the_windows_last_position():
    d, c, a = _flags(64, cand=(60, 63))
    _, state = _walk(100, d, c, a, what="last position")
    assert state["prev_variant_pos"] == 163 and state["num_variants"] == 2
    regions, _ = _walk(164, *_flags(40), state=state, what="the window after")
    assert regions == [(159, 165, 178)]


def test_window_of_200_cut_at_every_position():
    g = R.dense_walk(200)
    whole, whole_state = _walk(g["win_begin"], g["depth"], g["is_candidate"], g["is_anchor"], what="whole")
    assert len(whole) >= 8
    for k in range(0, 201):
        r1, s1 = capi.active_regions(g["win_begin"], _sites(g["sites"][:k]), g["is_candidate"][:k], g["is_anchor"][:k])
        r2, s2 = capi.active_regions(g["win_begin"] + k, _sites(g["sites"][k:]), g["is_candidate"][k:], g["is_anchor"][k:], s1 if k else None)
        got = [tuple(int(x) for x in r) for r in list(r1) + list(r2)]
        if k == 0:  # (an empty first window leaves the state as it was: is_beginning stays for the next)
            assert _state_dict(s1) == A.initial_state()
        assert got == whole and _state_dict(s2) == whole_state, k
    # ... and on a repeat-rich reference, at every position of a stretch around a region
    g = R.seeded_walk(1500, 32)
    whole, whole_state = _walk(g["win_begin"], g["depth"], g["is_candidate"], g["is_anchor"], what="seeded whole")
    at = whole[3][0] - g["win_begin"] - 10
    for k in range(at, at + 90):
        r1, s1 = capi.active_regions(g["win_begin"], _sites(g["sites"][:k]), g["is_candidate"][:k], g["is_anchor"][:k])
        r2, s2 = capi.active_regions(g["win_begin"] + k, _sites(g["sites"][k:]), g["is_candidate"][k:], g["is_anchor"][k:], s1)
        assert [tuple(int(x) for x in r) for r in list(r1) + list(r2)] == whole and _state_dict(s2) == whole_state, k


@functools.lru_cache(maxsize=None)
def _big_walk():
    return R.seeded_walk(WALK_CHUNK + 1, 34)


@pytest.mark.parametrize("n_pos", N_POS_EDGES + [WALK_CHUNK - 1, WALK_CHUNK, WALK_CHUNK + 1])
def test_walk_sizes_at_the_edges(n_pos):
    g = _big_walk()
    regions, _ = _walk(g["win_begin"], g["depth"][:n_pos], g["is_candidate"][:n_pos], g["is_anchor"][:n_pos], what="n_pos %d" % n_pos,
                       counts=[c for c, _ in g["sites"][:n_pos]])
    if n_pos >= 4096:
        assert len(regions) >= 8
    # ... with a candidate on the last position of the window, and the window after it
    d, c, a = list(g["depth"][:n_pos]), list(g["is_candidate"][:n_pos]), list(g["is_anchor"][:n_pos])
    d[-1], c[-1] = 20, 1
    _, state = _walk(g["win_begin"], d, c, a, what="n_pos %d, candidate last" % n_pos)
    _walk(g["win_begin"] + n_pos, *_flags(30), state=state, what="after n_pos %d" % n_pos)


def test_empty_window_and_region_cap_at_the_bound():
    capi.init(0)
    regions, state = capi.active_regions(50, _sites([]), [], [])
    assert len(regions) == 0 and _state_dict(state) == A.initial_state()
    # as many regions as positions allow: candidate pairs as close as the rules let them follow each other
    n = 16 * 40
    d, c, a = _flags(n, cand=tuple(k * 16 + j for k in range(40) for j in (0, 1)))
    want, _ = A.active_regions(10, d, c, a)
    assert len(want) == 40
    got, _ = capi.active_regions(10, _sites(list(zip([0] * n, d))), c, a, region_cap=capi.active_regions_bound(n))
    assert [tuple(int(x) for x in r) for r in got] == want
    with pytest.raises(capi.StrelkaAmdError, match="region_cap"):
        capi.active_regions(10, _sites(list(zip([0] * n, d))), c, a, region_cap=capi.active_regions_bound(n) - 1)
    # two positions, bound 2, and a region carried in by the state plus none of its own
    state = dict(A.initial_state(), is_beginning=0, active_region_start_pos=5, anchor_pos_following_prev_variant=12, prev_anchor_pos=29, prev_variant_pos=11, num_variants=3)
    regions, _ = _walk(30, *_flags(2), state=state, what="carried in")
    assert regions == [(5, 13, 31)]


def test_unreachable_state_is_an_error_return_not_a_fault():
    """createActiveRegion's assertion fails mid-window: the host entry fails with the message and leaves its outputs alone; the device
    entry raises the sticky flag, gives no region and hands the state back"""
    import torch
    capi.init(0)
    L = capi.lib()
    d, c, a = _flags(40)
    with pytest.raises(A.AssertionFailed):
        A.active_regions(50, d, c, a, R.UNREACHABLE_STATE)
    with pytest.raises(capi.StrelkaAmdError, match="createActiveRegion"):
        capi.active_regions(50, _sites(list(zip([0] * 40, d))), c, a, capi.ar_state(R.UNREACHABLE_STATE))
    assert L.sk_check_device_errors() == 0  # (the host entry took the flag with it)
    _walk(50, d[:8], c[:8], a[:8], state=R.UNREACHABLE_STATE, what="before the assertion's turn")
    if L.sk_broker_client():
        return
    p = lambda t: C.c_void_p(t.data_ptr())
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    t = [dev(_sites(list(zip([0] * 40, d))).view(np.int64)), dev(np.array(c, np.uint8)), dev(np.array(a, np.uint8)), dev(capi.ar_state(R.UNREACHABLE_STATE).view(np.int32))]
    d_out = torch.full((6,), 77, dtype=torch.int32, device="cuda")
    d_regions = torch.zeros(21 * 3, dtype=torch.int32, device="cuda")
    d_n = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    capi._check(L.sk_active_regions_dev(50, 40, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(d_out), p(d_regions), 21, p(d_n), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert L.sk_check_device_errors() != 0 and "createActiveRegion" in capi.last_error()
    assert L.sk_check_device_errors() == 0
    assert int(d_n.cpu()[0]) == 0
    assert d_out.cpu().numpy().tobytes() == capi.ar_state(R.UNREACHABLE_STATE).tobytes()


# ---- the whole pipeline ----------------------------------------------------------------------------------------------------------------------------------------


def test_recorded_finders():
    for f in R.golden()["finders"]:
        for k, reg in enumerate(f["regions"]):
            want, rows = _anchors(f["ref"], f["ref_offset"], reg["init_pos"], reg["init_span"], reg["m"], len(reg["anchors"]), reg["span_pos"],
                                  what="%s region %d" % (f["name"], k))
            assert want == reg["anchors"] and rows == reg["span_rows"]


def test_recorded_walks():
    capi.init(0)
    for w in R.golden()["walks"]:
        g = R.recorded_walk(w)
        n = len(g["sites"])
        anchor, _ = capi.ref_anchors(w["ref"], w["ref_offset"], g["win_begin"] + 1, None, g["win_begin"], n)
        assert anchor.tolist() == g["is_anchor"]
        regions, state = capi.active_regions(g["win_begin"], _sites(g["sites"]), g["is_candidate"], anchor)
        assert [tuple(int(x) for x in r) for r in regions] == g["regions"]
        assert _state_dict(state) == g["states"][-1]
        # ... and call by call: the state after every one of the first 300 calls
        state = None
        for i in range(300):
            regions, state = capi.active_regions(g["win_begin"] + i, _sites(g["sites"][i:i + 1]), g["is_candidate"][i:i + 1], anchor[i:i + 1], state)
            assert _state_dict(state) == g["states"][i], i
            assert [tuple(int(x) for x in r) for r in regions] == [r for r in g["regions"] if r[2] == g["win_begin"] + i + 1]


def _golden_chain_inputs():
    g = K.golden()
    win_begin = g["ref_offset"]  # the finder of a detector begun here starts at the segment's first position
    n_pos = 999 - win_begin
    return g, win_begin, n_pos


def _model_of_the_chain():
    g, win_begin, n_pos = _golden_chain_inputs()
    intake = M.read_intake(g["ref"], g["ref_offset"], g["reads"], g["low"], win_begin, n_pos, g["max_indel_size"])
    anchor, _ = A.ref_anchors(g["ref"], g["ref_offset"], win_begin + 1, None, win_begin, n_pos)
    regions, state = A.active_regions(win_begin, [d for _, d in intake["sites"]], intake["is_candidate"], anchor)
    return intake, anchor, regions, state


def _host_chain():
    g, win_begin, n_pos = _golden_chain_inputs()
    intake = capi.read_intake(g["ref"], g["ref_offset"], g["reads"], g["low"], win_begin, n_pos)
    anchor, _ = capi.ref_anchors(g["ref"], g["ref_offset"], win_begin + 1, None, win_begin, n_pos)
    regions, state = capi.active_regions(win_begin, intake["sites"], intake["is_candidate"], anchor)
    return anchor.tobytes() + regions.tobytes() + state.tobytes(), regions


def test_three_calls_on_one_stream_on_the_intakes_golden_reads():
    """sk_read_intake_dev -> sk_ref_anchors_dev -> sk_active_regions_dev on one stream, no host copy in between, against model-of-model"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    g, win_begin, n_pos = _golden_chain_inputs()
    intake, anchor, regions, state = _model_of_the_chain()
    assert len(regions) >= 3 and sum(anchor) > 100
    reads = g["reads"]
    n = len(reads)
    read_off, code, path_off, n_seg, path, pos = capi.pack_reads(reads)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    d_ref = dev(np.frombuffer(g["ref"].encode(), np.uint8).copy())
    t = [dev(read_off), dev(code), dev(path_off), dev(n_seg), dev(path.view(np.uint32)), dev(pos), dev(np.array(list(g["low"]) + [0], np.uint8))]
    n_segs = int(path_off[-1])
    cap = capi.read_intake_obs_bound(n_segs)
    d_reads = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_obs_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_obs = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    d_sites = torch.full((n_pos,), -1, dtype=torch.int64, device="cuda")
    d_cand = torch.full((n_pos,), 7, dtype=torch.uint8, device="cuda")
    scratch_bytes = L.sk_read_intake_scratch_bytes(n, n_segs, n_pos)
    d_scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    d_anchor = torch.full((n_pos,), 7, dtype=torch.uint8, device="cuda")
    d_state_in = dev(capi.ar_state_initial().view(np.int32))
    d_state_out = torch.zeros(6, dtype=torch.int32, device="cuda")
    region_cap = capi.active_regions_bound(n_pos)
    d_regions = torch.zeros(region_cap * 3, dtype=torch.int32, device="cuda")
    d_n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    opt = capi.intake_options()
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi._check(L.sk_read_intake_dev(p(d_ref), g["ref_offset"], len(g["ref"]), n, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]), C.byref(opt),
                                     win_begin, n_pos, p(d_reads), p(d_obs_off), p(d_obs), cap, p(d_sites), p(d_cand), p(d_scratch), scratch_bytes, st))
    capi._check(L.sk_ref_anchors_dev(p(d_ref), g["ref_offset"], len(g["ref"]), win_begin + 1, None, win_begin, n_pos, p(d_anchor), 0, None, None, st))
    capi._check(L.sk_active_regions_dev(win_begin, n_pos, p(d_sites), p(d_cand), p(d_anchor), p(d_state_in), p(d_state_out), p(d_regions), region_cap, p(d_n), st))
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    assert d_anchor.cpu().tolist() == anchor
    assert d_cand.cpu().numpy().astype(bool).tolist() == intake["is_candidate"]
    assert int(d_n.cpu()[0]) == len(regions)
    got = d_regions.cpu().numpy().view(capi.ACTIVE_REGION_DTYPE)[:len(regions)]
    assert [tuple(int(x) for x in r) for r in got] == regions
    assert _state_dict(d_state_out.cpu().numpy().view(capi.AR_STATE_DTYPE)) == state
    # the host entries, chained by the caller, give the same bytes
    host_bytes, host_regions = _host_chain()
    assert host_regions.tobytes() == got.tobytes()
    # state_out may be state_in: the next window, in place
    capi._check(L.sk_active_regions_dev(win_begin + n_pos, 0, None, None, None, p(d_state_out), p(d_state_out), p(d_regions), 1, p(d_n), st))
    torch.cuda.synchronize()
    assert int(d_n.cpu()[0]) == 0 and _state_dict(d_state_out.cpu().numpy().view(capi.AR_STATE_DTYPE)) == state


BROKER_CLIENT = r'''
import hashlib, json, sys
sys.path.insert(0, %r)
from strelka_amd import capi
from tests import test_active_region_detect as T
capi.init(0)
data, regions = T._host_chain()
print(json.dumps(dict(client=capi.lib().sk_broker_client(), digest=hashlib.sha256(data).hexdigest(), n_regions=int(len(regions)))))
'''


def test_chain_through_the_broker(tmp_path):
    capi.init(0)
    direct, regions = _host_chain()
    _, _, want_regions, _ = _model_of_the_chain()
    assert [tuple(int(x) for x in r) for r in regions] == want_regions
    env = dict(os.environ, STRELKA_AMD_BROKER="1", STRELKA_AMD_BROKER_SOCKET="sktest_" + uuid.uuid4().hex[:12], STRELKA_AMD_BROKER_LOG=str(tmp_path / "broker.log"),
               STRELKA_AMD_BROKER_IDLE_S="2")
    p = subprocess.run([sys.executable, "-c", BROKER_CLIENT % REPO], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    res = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert res["client"] == 1
    assert res["n_regions"] == len(regions) >= 3
    assert res["digest"] == hashlib.sha256(direct).hexdigest()
