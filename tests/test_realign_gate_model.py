"""The loop model of the realignment gate (tests/realign_gate_model.py) against vectors recorded from the reference's own
check_for_candidate_indel_overlap, get_alignment_zone, is_realignable, is_usable_indel and LogValuePair over its own IndelBuffer
(tests/golden/realign_gate, recorded by tools/golden/realign_gate_driver.cpp): field for field, for every read and key of every scene.
The file must hold a scene for every line of the gate the rules name; the test looks for each in the recorded data itself."""
import pytest

from tests import indel_candidates_model as CM
from tests import realign_gate_cases as G
from tests import realign_gate_model as GM

SCENES = [sc["name"] for sc in GM.golden()["scenes"]]


@pytest.fixture(scope="module")
def runs():
    """every recorded scene through the models, once: name -> (recorded scene, table keys, samples, realign_gate's result)"""
    out = {}
    for rec in GM.golden()["scenes"]:
        keys, cand, samples, res = GM.run_recorded(rec)
        out[rec["name"]] = (rec, keys, samples, res)
    return out


@pytest.mark.parametrize("name", SCENES)
def test_model_equals_the_recorded_scene(runs, name):
    rec, keys, samples, res = runs[name]
    doc = CM.scene_document(GM.candidate_scene(rec))
    want_keys, want_reads = GM.as_recorded(doc, res)
    assert len(want_keys) == len(rec["keys"]) and len(want_reads) == len(rec["reads"])
    for k, (w, r) in enumerate(zip(want_keys, rec["keys"])):
        assert w == r, k  # (the two logs of every sample as bit patterns)
    for w, r in zip(want_reads, rec["reads"]):
        assert w == r, (r["sample"], r["id"])


def _cases(runs):
    """every recorded (scene, read) with what the predicates below look at"""
    for rec, keys, samples, res in runs.values():
        doc = CM.scene_document(GM.candidate_scene(rec))
        ranges = {(s, i): (b, e) for s, i, b, e in rec["ranges"]}
        reads = {(s, r["id"]): r for s, sm in enumerate(doc["samples"]) for r in sm["reads"]}
        for rd in rec["reads"]:
            src = reads[(rd["sample"], rd["id"])]
            yield dict(rec=rec, keys=keys, rd=rd, src=src, zone=rd["zone"], mis=doc["max_indel_size"], range=ranges.get((rd["sample"], rd["id"])),
                       cand=[k["is_candidate"] for k in rec["keys"]])


def _in_range_reach(c, k):
    return k["pos"] >= c["zone"][0] - c["mis"]


def _interior(c, seg_type, length):
    path = c["src"]["path"]
    return any(t == seg_type and n == length for t, n in path[1:-1])


def _edge(c, seg_type, length):
    path = c["src"]["path"]
    return len(path) > 1 and any(t == seg_type and n == length for t, n in (path[0], path[-1]))


def _intersecting(c):
    return [i for i, k in enumerate(c["keys"]) if GM.intersects_breakpoints(c["zone"], k)]


RULES = {
    "a key whose right end is zone_begin": lambda c: any(k["type"] == CM.INDEL and k["del_len"] > 0 and GM.right_pos(k) == c["zone"][0] and _in_range_reach(c, k) for k in c["keys"]),
    "a key whose right end is zone_begin - 1": lambda c: any(k["type"] == CM.INDEL and k["del_len"] > 0 and GM.right_pos(k) == c["zone"][0] - 1 and _in_range_reach(c, k) for k in c["keys"]),
    "a key at pos == zone_end": lambda c: any(k["type"] == CM.INDEL and k["pos"] == c["zone"][1] for k in c["keys"]),
    "a key at pos == zone_end - 1": lambda c: any(k["type"] == CM.INDEL and k["pos"] == c["zone"][1] - 1 for k in c["keys"]) and c["rd"]["gate"] == 1,
    "a deletion whose left breakpoint lies before the zone and whose right lies inside":
        lambda c: any(k["type"] == CM.INDEL and k["pos"] < c["zone"][0] < GM.right_pos(k) < c["zone"][1] for k in c["keys"]) and c["rd"]["gate"] == 1,
    "an insertion at zone_begin": lambda c: any(k["type"] == CM.INDEL and k["del_len"] == 0 and k["ins"] and k["pos"] == c["zone"][0] for k in c["keys"]),
    "an insertion at zone_end": lambda c: any(k["type"] == CM.INDEL and k["del_len"] == 0 and k["ins"] and k["pos"] == c["zone"][1] for k in c["keys"]),
    "a MISMATCH key at zone_begin": lambda c: any(k["type"] == CM.MISMATCH and k["pos"] == c["zone"][0] for k in c["keys"]),
    "a MISMATCH key at zone_end": lambda c: any(k["type"] == CM.MISMATCH and k["pos"] == c["zone"][1] for k in c["keys"]),
    "a zone clamped at 0": lambda c: c["zone"][0] == 0 and c["src"]["pos"] - GM.unaligned_prefix([tuple(t) for t in c["src"]["path"]]) < 0,
    "the realign range equal to the zone": lambda c: c["range"] is not None and list(c["range"]) == c["zone"] and c["rd"]["gate"] == 1,
    "the realign range short by one position at its begin": lambda c: c["range"] is not None and c["range"][0] == c["zone"][0] + 1 and c["range"][1] >= c["zone"][1] and c["rd"]["gate"] == 0,
    "the realign range short by one position at its end": lambda c: c["range"] is not None and c["range"][1] == c["zone"][1] - 1 and c["range"][0] <= c["zone"][0] and c["rd"]["gate"] == 0,
    "an interior indel of max_indel_size": lambda c: _interior(c, CM.SEG_DELETE, c["mis"]) and c["rd"]["realignable"] == 1,
    "an interior indel of max_indel_size + 1": lambda c: _interior(c, CM.SEG_DELETE, c["mis"] + 1) and c["rd"]["realignable"] == 0,
    "an indel of max_indel_size at a path edge": lambda c: _edge(c, CM.SEG_INSERT, c["mis"]) and c["rd"]["realignable"] == 1,
    "an indel of max_indel_size + 1 at a path edge": lambda c: _edge(c, CM.SEG_INSERT, c["mis"] + 1) and c["rd"]["realignable"] == 1,
    "a non-candidate intersecting key before the first candidate": lambda c: c["rd"]["gate"] == 1 and len(c["rd"]["consulted"]) >= 2 and not c["cand"][c["rd"]["consulted"][0]],
    "two candidates": lambda c: c["rd"]["gate"] == 1 and any(c["cand"][i] and i > c["rd"]["consulted"][-1] for i in _intersecting(c)),
    "a read in a noise set and a support set of one key":
        lambda c: any(c["rd"]["id"] in k["samples"][c["rd"]["sample"]]["ids"][3] and any(c["rd"]["id"] in ids for ids in k["samples"][c["rd"]["sample"]]["ids"][:3]) for k in c["keys"]),
    "a sub-mapped read": lambda c: c["src"]["iat"] == CM.IAT_SUBMAP and len(c["rd"]["member"]) > 0,
    "a read that passes": lambda c: c["rd"]["gate"] == 1,
    "a read no candidate lets pass": lambda c: c["rd"]["gate"] == 0 and c["rd"]["realignable"] == 1 and len(c["rd"]["consulted"]) > 0,
    "a log of a rate the error factor scaled": lambda c: c["rec"]["name"].endswith("@germline") and len(c["keys"]) > 0,
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_the_file_holds_a_scene_for_every_rule(runs, rule):
    assert any(RULES[rule](c) for c in _cases(runs)), rule


def test_the_recorded_consulted_sets_fold_into_the_marks(runs):
    """rule G4 over a whole scene: the union of what the recorded reads' gates asked is the model's gate_consulted"""
    n = 0
    for rec, keys, samples, res in runs.values():
        marks = [0] * len(rec["keys"])
        for rd in rec["reads"]:
            for k in rd["consulted"]:
                marks[k] = 1
        assert marks == [k["gate_consulted"] for k in res["keys"]], rec["name"]
        n += sum(marks)
    assert n > 0


def test_rule_functions_on_crafted_inputs():
    M, I, D, S, H = G.M, G.I, G.D, G.S, G.H
    assert GM.alignment_zone(100, [(S, 5), (M, 20), (I, 2), (S, 3)], 30) == (95, 125) and GM.alignment_zone(3, [(S, 10), (M, 5)], 15) == (0, 8)
    assert GM.alignment_zone(100, [(H, 9), (M, 20), (D, 7), (M, 1)], 21) == (100, 128) and GM.alignment_zone(50, [(I, 4), (S, 2)], 6) == (44, 56)
    assert GM.is_overmax([(M, 5), (D, 9), (M, 5)], 8) and not GM.is_overmax([(M, 5), (D, 8), (M, 5)], 8) and not GM.is_overmax([(I, 9), (M, 5)], 8) and not GM.is_overmax([(D, 9)], 8)
    keys = [G.key(90, del_len=10), G.key(95, del_len=4), G.key(100, ins="A"), G.key(120, del_len=1)]
    assert GM.range_iterator(keys, 100, 120, 49) == (0, 3) and GM.range_iterator(keys, 100, 120, 9) == (2, 3) and GM.range_iterator(keys, 100, 121, 5) == (2, 4)
    assert GM.range_iterator(keys, 101, 120, 49) == (3, 3)  # the right ends (100, 99 and the insertion's 100) lie before 101
    assert [GM.intersects_breakpoints((100, 120), k) for k in keys] == [False, False, False, False]
    assert [GM.intersects_breakpoints((99, 121), k) for k in keys] == [True, False, True, True]  # (95 + 4 == 99: not inside)
    with pytest.raises(GM.Refused):
        GM.observed_lists([G.key(10, del_len=1, ids=[[[5], [], [], []]])], 0, [1, 2])
    with pytest.raises(GM.Refused):
        GM.realign_gate([], [], [dict(reads=[G.read(0, [(M, 5)])] * 2, align_id=[3, 3])], 49)
    assert GM.log_rates([CM.double_bits(0.0), CM.double_bits(1.0), 0, 0]) == [CM.double_bits(float("-inf")), 0]
