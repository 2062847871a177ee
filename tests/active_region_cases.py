"""Inputs of the active-region tests, shared by the model tests (tests/test_active_region_detect_model.py), the device tests
(tests/test_active_region_detect.py) and smoke(): the vectors recorded from the reference and the seeded walk inputs.  Imports
neither the product nor a device."""
import functools
import json
import os

import numpy as np

from tests import anchor_model as A
from tests import intake_cases as K
from tests import intake_model as M

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "active_region_detect")
# two variants counted and no anchor after them yet, but a start beyond the window: createActiveRegion's assertion (:318) fails at the
# first event more than 13 past position 45, not at once
UNREACHABLE_STATE = dict(is_beginning=0, active_region_start_pos=100, anchor_pos_following_prev_variant=-1, prev_anchor_pos=44, prev_variant_pos=45, num_variants=2)


@functools.lru_cache(maxsize=None)
def golden():
    """-> dict(finders, walks): what tools/golden/active_region_driver.cpp recorded (its header says what each field is)"""
    with open(os.path.join(GOLDEN_DIR, "finder.json")) as f:
        finders = json.load(f)["items"]
    with open(os.path.join(GOLDEN_DIR, "walk.json")) as f:
        walks = json.load(f)["items"]
    return dict(finders=finders, walks=walks)


def recorded_walk(item):
    """a recorded walk in the form the model and the device take and give
    -> dict(win_begin, sites, depth, is_candidate, is_anchor, regions [(begin, end, made_at)], states [dict per call])"""
    calls = item["calls"]
    win_begin = item["win_begin"]
    regions = [(c[9], c[10], win_begin + i + 1) for i, c in enumerate(calls) if c[9] >= 0]
    return dict(win_begin=win_begin, sites=[tuple(s) for s in item["sites"]], depth=[s[1] for s in item["sites"]], is_candidate=[c[0] for c in calls],
                is_anchor=[c[2] for c in calls], regions=regions, states=[dict(zip(A.STATE_FIELDS, c[3:9])) for c in calls])


def walk_sites(n, rng, candidate_rate):
    """(variant count, depth) per position: mostly quiet, candidates alone and in clusters a few positions apart, depth-zero stretches
    -- inside clusters too, where a depth-zero position counts as a candidate"""
    sites = []
    while len(sites) < n:
        r = rng.random()
        if r < 0.01:
            sites += [(0, 0)] * int(rng.integers(1, 30))
        elif r < 0.01 + candidate_rate:
            for _ in range(int(rng.integers(1, 4))):
                depth = int(rng.integers(8, 40))
                sites.append((int(depth * rng.uniform(0.4, 1.0)) + 1, depth + 1))
                for _ in range(int(rng.integers(0, 16))):
                    sites.append((0, 0) if rng.random() < 0.07 else (int(rng.random() < 0.2), int(rng.integers(10, 40))))
        else:
            sites.append((int(rng.integers(0, 2)), int(rng.integers(10, 40))))
    return sites[:n]


def walk_flags(ref, ref_offset, win_begin, sites, init_pos=None):
    """what the intake's R4 and the finder give for `sites`, by the models -> (depth, is_candidate, is_anchor); a fresh detector's finder
    is initialised at its first call's position, win_begin + 1"""
    depth = [d for _, d in sites]
    cand = [1 if M.is_candidate_variant(M.ref_char(ref, ref_offset, win_begin + i), c, d) else 0 for i, (c, d) in enumerate(sites)]
    anchor, _ = A.ref_anchors(ref, ref_offset, win_begin + 1 if init_pos is None else init_pos, None, win_begin, len(sites))
    return depth, cand, anchor


@functools.lru_cache(maxsize=None)
def seeded_walk(n, seed, candidate_rate=0.04, win_begin=500, ref_offset=400):
    """-> dict(ref, ref_offset, win_begin, sites, depth, is_candidate, is_anchor) over a repeat-rich reference"""
    rng = np.random.default_rng(seed)
    ref = K.repeat_rich_reference(win_begin - ref_offset + n + 150, rng)
    sites = walk_sites(n, rng, candidate_rate)
    depth, cand, anchor = walk_flags(ref, ref_offset, win_begin, sites)
    return dict(ref=ref, ref_offset=ref_offset, win_begin=win_begin, sites=sites, depth=depth, is_candidate=cand, is_anchor=anchor)


@functools.lru_cache(maxsize=None)
def dense_walk(n=200, win_begin=300):
    """a short window with a region every 24 positions: two candidates three apart (in every second cluster a depth-zero position
    between them, which counts), then 20 quiet positions (in every second cluster one of depth zero, which does not count), over a
    reference without repeats, so that every position is a ring anchor -> the form seeded_walk gives"""
    ref = thue(win_begin + n + 150, "ACG")
    sites = []
    for i in range(n):
        k, at = divmod(i, 24)
        if at in (0, 3):
            sites.append((9 + k, 20 + k))
        elif (at == 1 and k % 2 == 0) or (at == 20 and k % 2 == 1):
            sites.append((0, 0))
        else:
            sites.append((at % 2, 25))
    depth, cand, anchor = walk_flags(ref, 0, win_begin, sites)
    return dict(ref=ref, ref_offset=0, win_begin=win_begin, sites=sites, depth=depth, is_candidate=cand, is_anchor=anchor)


def thue(n, letters):
    """the first n letters of Thue's square-free word (a -> abc, b -> ac, c -> b) over three given letters: no block occurs twice in a
    row, so no position of it lies in a repeat of any unit length"""
    w = "a"
    while len(w) < n:
        w = "".join({"a": "abc", "b": "ac", "c": "b"}[c] for c in w)
    return "".join(letters["abc".index(c)] for c in w[:n])


TRACT_AT, TRACT_REF_LEN = 400, 800


def _with_tract(unit, total):
    bg = thue(TRACT_REF_LEN, "ACG")
    return bg[:TRACT_AT] + (unit * (total // len(unit) + 1))[:total] + bg[TRACT_AT + total:]


# where in Thue's word over TGC a unit of u bases begins that meets the background cleanly at TRACT_AT (found once by trying 0, 1, ...;
# tests/test_active_region_detect_model.py checks the property on the model): a tract of 2u - 1 bases of it (u = 1: 2) leaves every
# position an anchor and one of 2u bases (u = 1: 3) unsets exactly the tract; for u = 51 three units leave every position an anchor
_UNIT_BEGIN = {2: 5, 3: 3, 7: 6, 49: 0, 50: 111, 51: 31}


def tract_unit(u):
    """a unit of u bases, itself square-free"""
    return "T" if u == 1 else thue(u + _UNIT_BEGIN[u], "TGC")[_UNIT_BEGIN[u]:_UNIT_BEGIN[u] + u]


def tract_reference(u, total):
    """the square-free background (800 bases, offset 0) with a period-u tract of `total` bases at position TRACT_AT"""
    return _with_tract(tract_unit(u), total)
