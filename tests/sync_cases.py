"""Inputs shared by the synchroniser's tests: the vectors recorded from the reference's ActiveRegionDetector (tests/golden/sync_regions/,
made by tools/golden/make_sync_regions_golden.py), replayed through tests/sync_model.py, and seeded windows.

This module does not import the product."""
import functools
import glob
import json
import os

import numpy as np

from tests import anchor_model as A
from tests import sync_model as S

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sync_regions")
ID_SCAN = 260  # the driver reads the id map over this many positions below _prevActiveRegionEnd


@functools.lru_cache(maxsize=None)
def golden():
    """the recorded items, by file name"""
    items = []
    for path in sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.json"))):
        with open(path) as f:
            items += json.load(f)["items"]
    return items


def decode_row(row, n_samples, rel, last):
    """a recorded row "samples|region|ids" -> (the state it stands for, without the sample mask; the id map's runs); last: [the samples'
    states of the row before, that row's position], updated here ('=': the same again; '+': the same with the start and the previous
    anchor, where set, moved along with the call; '^': with the previous anchor alone moved)"""
    def pos(x):
        return -1 if x < 0 else rel - x
    parts = row.split("|")
    samples = []
    for k, text in enumerate(parts[0].split(";")):
        if text in "=+^":
            d = dict(last[0][k])
            if text != "=":
                for f in ("active_region_start_pos", "prev_anchor_pos") if text == "+" else ("prev_anchor_pos",):
                    d[f] = d[f] + rel - last[1] if d[f] >= 0 else d[f]
        else:
            r = [int(x) for x in text.lstrip("B").split(",")]
            d = dict(is_beginning=int(text.startswith("B")), active_region_start_pos=pos(r[0]), anchor_pos_following_prev_variant=r[1], prev_anchor_pos=pos(r[2]),
                     prev_variant_pos=r[3], num_variants=r[4])
        samples.append(d)
    assert len(samples) == n_samples
    last[0], last[1] = [dict(d) for d in samples], rel
    sync = [int(x) for x in parts[1].split(",")]
    runs = [tuple(int(x) for x in run.split(",")) for run in parts[2].split(";")] if parts[2] else []
    return dict(samples=samples, sync_begin=sync[0], sync_end=sync[1], prev_end=sync[2]), runs


def id_runs(ids, hi):
    """the runs [from, to, id] of the id map over [hi - ID_SCAN, hi), as the driver prints them"""
    runs, run, start = [], -1, 0
    for p in range(hi - ID_SCAN, hi + 1):
        v = ids.get(p, -1) if 0 <= p < hi else -1
        if v == run:
            continue
        if run != -1:
            runs.append((start, p, run))
        run, start = v, p
    return runs


def _comparable(state, n_samples):
    return dict(samples=state["samples"][:n_samples], sync_begin=state["sync_begin"], sync_end=state["sync_end"], prev_end=state["prev_end"])


def replay(item, check=False):
    """The item's operations through the model, chained through the state.  -> dict(regions, notes, windows): a window per step or clear
    operation with everything a call of sk_sync_active_regions takes and gives.  check: assert the model equals the recording after every
    call and after every clear()"""
    n_samples, default_ploidy = item["n_samples"], item["default_ploidy"]
    marks = [dict() for _ in range(n_samples)]
    state, ids = S.initial_state(n_samples), {}
    regions, notes, windows = [], [], []
    last_pos, last_row = 0, [None, 0]
    for op in item["ops"]:
        if op["op"] == "ploidy":
            marks[op["sample"]][op["pos"]] = op["ploidy"]
            continue
        mark_lists = [sorted(m.items()) for m in marks]
        if op["op"] == "step":
            win_begin, n = op["win_begin"], len(op["anchors"])
            anchor = [int(c) for c in op["anchors"]]
            cand = [[int(c) & 1 for c in f] for f in op["flags"]]
            depth = [[0 if int(c) & 2 else 20 for c in f] for f in op["flags"]]
            det = S.Detector(win_begin, depth, cand, anchor, mark_lists, default_ploidy, state)
            det.ids = ids
            for i in range(n):
                pos = win_begin + 1 + i
                before = det.prev_end
                det.update_end_position(pos)
                if check:
                    want, runs = decode_row(op["calls"][i], n_samples, pos, last_row)
                    assert _comparable(det.state(), n_samples) == want, "%s: call %d" % (item["name"], pos)
                    assert (id_runs(ids, det.prev_end) if det.prev_end != before else []) == runs, "%s: the id map after call %d" % (item["name"], pos)
            last_pos = win_begin + n
            win = dict(win_begin=win_begin, depth=depth, cand=cand, anchor=anchor, do_clear=False, buf_begin=None, buf_end=None)
        else:
            det = S.Detector(last_pos, [[] for _ in range(n_samples)], [[] for _ in range(n_samples)], [], mark_lists, default_ploidy, state)
            det.ids = ids
            before = det.prev_end
            branches = []
            for s, d in enumerate(det.samples):  # which of closeActiveRegionDetector's branches each sample takes (:419-435)
                undetermined = d._active_region_start_pos < 0 and d._anchor_pos_following_prev_variant < 0
                branches.append("none" if d._is_beginning or d._num_variants < A.MIN_NUM_VARIANTS_PER_REGION else
                                "kept" if undetermined and not op["buf_begin"][s] < op["buf_end"][s] else "made")
            det.clear(op["buf_begin"], op["buf_end"])
            if check:
                want, runs = decode_row(op["after"], n_samples, op["rel"], last_row)
                assert _comparable(det.state(), n_samples) == want, "%s: clear()" % item["name"]
                assert (id_runs(ids, det.prev_end) if det.prev_end != before else []) == runs, "%s: the id map after clear()" % item["name"]
            win = dict(win_begin=last_pos, depth=[[] for _ in range(n_samples)], cand=[[] for _ in range(n_samples)], anchor=[], do_clear=True,
                       buf_begin=op["buf_begin"], buf_end=op["buf_end"], branches=branches, sync_open=state["sync_end"] != 0)
        win.update(marks=mark_lists, default_ploidy=default_ploidy, state_in=state, state_out=det.state(), regions=det.regions,
                   region_id=[ids.get(p, -1) for p in range(win["win_begin"], win["win_begin"] + len(win["anchor"]))])
        state = det.state()
        regions += det.regions
        notes += det.notes
        windows.append(win)
    return dict(regions=regions, notes=notes, windows=windows)


def coverage():
    """what the fixture holds, counted through the model (which test_sync_regions_model pins to the recording call by call)"""
    c = dict(merged_from_two_or_more=0, delayed_by_another_sample=0, own_merges=0, over_250=0, ploidies_differ=0, sample_counts=set(), from_zero=0,
             inside_segment=0, clear_branches=set(), clear_with_open_region=0, regions=0)
    for item in golden():
        r = replay(item)
        c["sample_counts"].add(item["n_samples"])
        first = next(w for w in r["windows"] if not w["do_clear"])
        c["from_zero" if first["win_begin"] == 0 else "inside_segment"] += 1
        c["regions"] += len(r["regions"])
        for g, note in zip(r["regions"], r["notes"]):
            c["merged_from_two_or_more"] += bin(g["sample_mask"]).count("1") >= 2
            c["delayed_by_another_sample"] += g["closed_at"] > g["end"] + S.MAX_ASSEMBLY_PADDING and note["delayed_by_other"]
            c["own_merges"] += note["own_merge"]
            c["over_250"] += g["end"] - g["begin"] > S.MAX_REF_SPAN_TO_BYPASS_ASSEMBLY
            c["ploidies_differ"] += len(set(g["ploidy"])) > 1
        for w in r["windows"]:
            if w["do_clear"]:
                c["clear_branches"] |= set(w["branches"])
                c["clear_with_open_region"] += w["sync_open"]
    c["sample_counts"] = sorted(c["sample_counts"])
    c["clear_branches"] = sorted(c["clear_branches"])
    return c


# ---- seeded windows -----------------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def seeded(n_samples, n_pos, seed, win_begin=300):
    """A window of clusters the samples share with shifts of their own, chains that hold the others' regions open, depth-zero and
    no-anchor stretches, and ploidy marks on some regions' ends -> dict(win_begin, depth, cand, anchor, marks)"""
    rng = np.random.default_rng(seed)
    anchor = (rng.random(n_pos) < 0.9).astype(np.uint8)
    depth = np.full((n_samples, n_pos), 20, np.int64)
    cand = np.zeros((n_samples, n_pos), np.uint8)
    at = int(rng.integers(0, 30))
    while at < n_pos:
        if rng.random() < 0.15:
            anchor[at:at + int(rng.integers(5, 40))] = 0
        for s in range(n_samples):
            if rng.random() >= 0.6:
                continue
            p = at + int(rng.integers(-8, 9))
            for _ in range(int(rng.integers(7, 14)) if rng.random() < 0.25 else int(rng.integers(1, 5))):
                if 0 <= p < n_pos:
                    cand[s, p] = 1
                p += int(rng.integers(1, 14))
        if rng.random() < 0.2:
            s, p = int(rng.integers(0, n_samples)), at + int(rng.integers(5, 25))
            depth[s, p:p + int(rng.integers(2, 20))] = 0
        if rng.random() < 0.03:  # a chain long enough for a region over 250 positions
            s = int(rng.integers(0, n_samples))
            cand[s, at:at + 300:11] = 1
        at += int(rng.integers(30, 70))
    cand[depth == 0] = 1  # (the intake flags every depth-zero position whose reference is not N)
    depth, cand, anchor = depth.tolist(), cand.tolist(), anchor.tolist()
    regions, _, _ = S.sync_active_regions(win_begin, depth, cand, anchor)
    marks = [dict() for _ in range(n_samples)]
    for k, g in enumerate(regions):
        s = k % n_samples
        if k % 3 == 0:
            marks[s][g["begin"]] = marks[s][g["end"] - 1] = 1
        elif k % 3 == 1:
            marks[s][g["begin"]] = 1
    return dict(win_begin=win_begin, depth=depth, cand=cand, anchor=anchor, marks=[sorted(m.items()) for m in marks])
