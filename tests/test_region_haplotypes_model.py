"""The loop model of the per-read haplotype store and the counting path (tests/haplotype_model.py) reproduces every field recorded from
the reference (tests/golden/region_haplotypes/, made by tools/golden/make_region_haplotypes_golden.py), and gives the hand-computed
values of crafted cases for each of its rules.  No device, no product."""
import numpy as np
import pytest

from tests import haplotype_model as H
from tests import intake_model as M
from tests import region_haplotype_cases as R

MS, IN, DE, SC, HC = R.MS, R.IN, R.DE, R.SC, R.HC


def _scene(name):
    return next(s for s in R.golden() if s["name"] == name)


def _expected_status(sc, g):
    if g["begin"] < sc["buf_begin"] or g["end"] > sc["buf_end"] or g["end"] - g["begin"] > 250:
        return H.BYPASSED
    if g["n_reads_aligned"] == 0:
        return H.NO_READS
    return H.COUNTED if g["counted"] else H.TOO_FEW_COVERING


@pytest.mark.parametrize("name", [s["name"] for s in R.golden()])
def test_model_reproduces_the_recorded_scene(name):
    sc = _scene(name)
    buf, _ = H.build_buffer(sc["ref"], sc["ref_offset"], sc["reads"], sc["low"], sc["fwd"], sc["max_indel_size"])
    for g in sc["regions"]:
        what = "%s [%d, %d) ploidy %d" % (name, g["begin"], g["end"], g["ploidy"])
        n_aligned, segments = H.get_read_segments(buf, g["begin"], g["end"], sc["buf_begin"], sc["buf_end"])
        assert n_aligned == g["n_reads_aligned"], what
        assert [[i, s] for i, s in segments] == g["segments"], what
        rec = H.region_haplotypes(sc["ref"], sc["ref_offset"], sc["reads"], sc["low"], sc["fwd"], [(g["begin"], g["end"])], sc["buf_begin"], sc["buf_end"],
                                  g["ploidy"], sc["max_indel_size"], buf=buf)[0]
        assert rec["status"] == _expected_status(sc, g) and rec["reason"] == H.DECLINE_NONE, what
        if rec["status"] != H.BYPASSED:
            assert rec["n_reads_aligned"] == g["n_reads_aligned"], what
        if rec["status"] in (H.COUNTED, H.TOO_FEW_COVERING):
            assert rec["n_reads_covering"] == len(g["segments"]), what
        assert [dict(seq=h["seq"], support=h["support"]) for h in rec["haps"]] == g["selected"], what
        for h in rec["haps"]:
            assert h["count"] == len(h["support"]) and h["is_reference"] == int(h["seq"] == sc["ref"][g["begin"] - sc["ref_offset"]:g["end"] - sc["ref_offset"]])


def test_the_recorded_vectors_hold_the_cases_they_were_made_for():
    sel = {(s["name"], g["ploidy"]): [len(h["support"]) for h in g["selected"]] for s in R.golden() for g in s["regions"][:2]}
    assert sel[("tie_15ref_12_12", 2)] == [15, 12, 12] and sel[("tie_15ref_12_12", 1)] == [15]
    assert sel[("tie_15ref_12_12_12", 2)] == [15]
    assert sel[("tie_15alt_12_12", 2)] == [15] and sel[("tie_15alt_12ref_12", 2)] == [15, 12, 12]
    assert sel[("tie_lengths_prefix", 1)] == [8, 8]
    assert sel[("phasing_right_run11_reverse_only", 2)] == [12] and sel[("phasing_right_run10_reverse_only", 2)] == [12, 5]
    assert sel[("phasing_left_run11_forward_only", 2)] == [12] and sel[("phasing_left_run10_forward_only", 2)] == [12, 4]
    assert sel[("phasing_right_run11_mixed_strands", 2)] == [12, 4]
    assert sel[("phasing_left_stops_at_the_strings_start", 2)] == [12, 4] and sel[("phasing_left_run12_from_the_strings_start", 2)] == [12]
    counted = {s["name"]: s["regions"][0]["counted"] for s in R.golden() if s["name"].startswith("coverage")}
    assert counted == dict(coverage_13_of_20=1, coverage_12_of_20=0, coverage_65_of_100=1, coverage_64_of_100=0)
    # the prefix sorts first: the reference segment without its last base, then the reference segment
    g = _scene("tie_lengths_prefix")["regions"][1]
    assert g["selected"][1]["seq"][:-1] == g["selected"][0]["seq"]
    # the top haplotype is not the reference
    sc = _scene("top_not_reference")
    g = sc["regions"][1]
    assert g["selected"][0]["seq"] != sc["ref"][100:108] and g["selected"][1]["seq"] == sc["ref"][100:108]


# ---- the store, rule by rule: hand-computed -----------------------------------------------------------------------------------------------------------


def _store(reads, low=None):
    buf, _ = H.build_buffer(R.REF, R.REF_OFFSET, reads, low or [0] * len(reads), [1] * len(reads))
    return buf


def _ref(b, e):
    return R.REF[b - R.REF_OFFSET:e - R.REF_OFFSET]


def test_store_match_mismatch_and_low_mapq():
    buf = _store([R.read(200, [(MS, 5)], subs={202: "N"}), R.read(200, [(MS, 5)], subs={203: None})], low=[0, 1])
    assert [buf.variant_info[(0, p)] for p in range(200, 205)] == [H.MATCH, H.MATCH, H.MISMATCH, H.MATCH, H.MATCH]
    assert buf.get_haplotype_base(0, 202) == ("N", False) and buf.get_haplotype_base(0, 201) == (R.REF[101], False)
    assert not any(k[0] == 1 for k in buf.variant_info)  # a low-MAPQ read registers nothing
    assert buf.position_to_align_ids[200] == [0]


def test_store_deletion_insertion_and_insertion_over_a_mismatch():
    buf = _store([R.read(200, [(MS, 5), (DE, 2), (MS, 5)]), R.read(200, [(MS, 5), (IN, 2), (MS, 5)], ins=["GA"]),
                  R.read(200, [(MS, 5), (IN, 2), (MS, 5)], subs={204: None}, ins=["GA"])])
    assert buf.variant_info[(0, 205)] == buf.variant_info[(0, 206)] == H.DELETE and buf.get_haplotype_base(0, 205) == ("", False)
    assert buf.variant_info[(1, 204)] == H.INSERT and buf.get_haplotype_base(1, 204) == (R.REF[104] + "GA", False)
    assert buf.variant_info[(2, 204)] == H.MISMATCH_INSERT and buf.get_haplotype_base(2, 204) == (R.other(R.REF[104]) + "GA", False)
    assert (1, 205) in buf.variant_info and buf.variant_info[(1, 205)] == H.MATCH  # the insert sits on 204 alone


def test_store_soft_clips_and_what_registers_nothing():
    buf = _store([R.read(200, [(SC, 3), (MS, 5), (SC, 2)]), R.read(200, [(MS, 5), (IN, 2), (DE, 3), (MS, 5)]), R.read(200, [(MS, 5), (DE, 50), (MS, 5)]),
                  R.read(200, [(IN, 2), (MS, 5), (DE, 2)]), R.read(200, [(HC, 4), (MS, 5)])])
    assert buf.variant_info[(0, 199)] == H.SOFT_CLIP and buf.variant_info[(0, 205)] == H.SOFT_CLIP
    assert buf.get_haplotype_base(0, 199) == ("TTT", True) and buf.get_haplotype_base(0, 205) == ("TT", True)
    assert sorted(p for (i, p) in buf.variant_info if i == 1) == list(range(200, 205)) + list(range(208, 213))  # a swap: 205..207 a hole
    assert sorted(p for (i, p) in buf.variant_info if i == 2) == list(range(200, 205)) + list(range(255, 260))  # above max_indel_size
    assert sorted(p for (i, p) in buf.variant_info if i == 3) == list(range(200, 205))                         # edge indels
    assert sorted(p for (i, p) in buf.variant_info if i == 4) == list(range(200, 205))                         # a hard clip


def test_read_segments_conditions():
    reads = [R.read(190, [(MS, 30)]),                       # 0 covers
             R.read(201, [(MS, 30)]),                       # 1 not registered at begin
             R.read(190, [(MS, 15)]),                       # 2 not registered at end - 1
             R.read(203, [(SC, 3), (MS, 30)]),              # 3 soft-clipped at 202
             R.read(190, [(MS, 30)], subs={205: "N"}),      # 4 an N
             R.read(190, [(MS, 10), (DE, 6), (MS, 10)]),    # 5 the whole region deleted: an empty string
             R.read(190, [(MS, 13), (IN, 1), (DE, 2), (MS, 10)]),  # 6 a hole inside: registered at both ends, shorter
             R.read(300, [(MS, 30)])]                       # 7 elsewhere
    buf = _store(reads)
    n_aligned, segments = H.get_read_segments(buf, 200, 206, 100, 500)
    assert n_aligned == 7
    assert segments == [(0, _ref(200, 206)), (6, _ref(200, 203) + _ref(205, 206))]
    # outside the read buffer's range positions are skipped (:204)
    assert H.get_read_segments(buf, 200, 206, 201, 500) == (7, [])


def test_status_rules():
    reads = R.plain(13) + [R.read(204, [(MS, 30)])] * 7
    c = R.case(reads, [(200, 210), (99, 110), (490, 501), (200, 450), (200, 451), (400, 410)])
    rec = R.model(c)
    # 250 positions are not bypassed (no read reaches their end: none covers), 251 are
    assert [r["status"] for r in rec] == [H.COUNTED, H.BYPASSED, H.BYPASSED, H.TOO_FEW_COVERING, H.BYPASSED, H.NO_READS]
    assert (rec[0]["n_reads_aligned"], rec[0]["n_reads_covering"]) == (20, 13)
    assert (rec[3]["n_reads_aligned"], rec[3]["n_reads_covering"]) == (20, 0)
    c = R.case(R.plain(12) + [R.read(204, [(MS, 30)])] * 8, [(200, 210)])
    assert R.model(c)[0]["status"] == H.TOO_FEW_COVERING
    # the comparison is float32's: 0.65f * 20 rounds to 13, so 13 of 20 is not below it
    assert not (np.float32(13) < np.float32(0.65) * np.float32(20)) and 13 < 0.65 * 20 + 1e-9


def test_grouping_order_and_selection_by_hand():
    a, b, c = {202: None}, {204: None}, {206: None}
    ref = _ref(200, 208)

    def hap(subs):
        return "".join(R.other(ch) if 200 + i in subs else ch for i, ch in enumerate(ref))
    case = R.case(R.plain(15) + R.plain(12, a) + R.plain(12, b), [(200, 208)])
    rec = R.model(case)[0]
    tied = sorted([hap(a), hap(b)])  # equal counts keep std::map order
    assert [(h["seq"], h["count"], h["is_reference"]) for h in rec["haps"]] == [(ref, 15, 1), (tied[0], 12, 0), (tied[1], 12, 0)]
    assert rec["haps"][0]["support"] == list(range(15))
    case = R.case(R.plain(15) + R.plain(12, a) + R.plain(12, b) + R.plain(12, c), [(200, 208)])
    assert [h["count"] for h in R.model(case)[0]["haps"]] == [15]
    case = R.case(R.plain(15, c) + R.plain(12, a) + R.plain(12, b), [(200, 208)])  # no reference among them: the tie is dropped
    assert [h["seq"] for h in R.model(case)[0]["haps"]] == [hap(c)]
    case = R.case(R.plain(15) + R.plain(12, a) + R.plain(12, b), [(200, 208)], ploidy=1)
    assert [h["count"] for h in R.model(case)[0]["haps"]] == [15]
    case = R.case(R.plain(2) + R.plain(2, a), [(200, 208)])  # nothing reaches MinHaplotypeCount: counted, nothing selected
    rec = R.model(case)[0]
    assert rec["status"] == H.COUNTED and rec["haps"] == [] and rec["n_reads_covering"] == 4


def test_phasing_noise_filter_by_hand():
    fwd = {i: i < 3 for i in range(8)}
    hap1 = "GT" + "A" * 10 + "CG"
    right = "GA" + "A" * 10 + "CG"  # the changed base begins a run of 11 to its right
    left = "GT" + "A" * 10 + "AG"   # ... ends a run of 11 to its left
    groups = lambda h2, ids: {hap1: [6, 7], h2: ids}  # (a read is in one group: no duplicates)
    f = H.is_filter_second_haplotype_as_sequencer_phasing_noise
    assert f(fwd, groups(right, [3, 4, 5]), hap1, right)            # no forward read: rightwards, 11 > 10
    assert not f(fwd, groups(right, [0, 1, 2]), hap1, right)        # all forward: leftwards, the run is 1 ('G' before it)
    assert f(fwd, groups(left, [0, 1]), hap1, left)                 # all forward: leftwards, 11
    assert not f(fwd, groups(left, [3, 4]), hap1, left)             # no forward read: rightwards, 1
    assert not f(fwd, groups(right, [2, 3]), hap1, right)           # mixed strands
    assert not f(fwd, {"GT" + "A" * 9 + "CCG": [6, 7], "GA" + "A" * 9 + "CCG": [3, 4]}, "GT" + "A" * 9 + "CCG", "GA" + "A" * 9 + "CCG")  # 10 is not above 10
    # the leftward loop stops at the string's first character without counting it: a run of 11 from the start gives 10
    assert not f(fwd, {"A" * 10 + "CG": [0], "A" * 10 + "AG": [1]}, "A" * 10 + "CG", "A" * 10 + "AG")
    assert f(fwd, {"A" * 11 + "CG": [0], "A" * 11 + "AG": [1]}, "A" * 11 + "CG", "A" * 11 + "AG")
    assert not f(fwd, groups(hap1[:-1], [3]), hap1, hap1[:-1]) and not f(fwd, groups("CA" + hap1[2:], [3]), hap1, "CA" + hap1[2:])  # condition 1


def test_decline_rules():
    assert R.model(R.groups_case(16))[0]["status"] == H.COUNTED
    rec = R.model(R.groups_case(17))[0]
    assert (rec["status"], rec["reason"], rec["n_reads_covering"], rec["haps"]) == (H.DECLINED, H.DECLINE_GROUPS, 51, [])
    assert R.model(R.spread_case(999))[0]["status"] == H.COUNTED
    rec = R.model(R.spread_case(1000))[0]
    assert (rec["status"], rec["reason"], rec["n_reads_aligned"]) == (H.DECLINED, H.DECLINE_READ_INDEX_SPREAD, 6)
    long_read = R.read(150, [(MS, 55), (DE, 900), (MS, 45)], ref=R.REF, ref_offset=R.REF_OFFSET)  # first and last position 999 apart, then 1 000
    c = R.case(R.plain(3) + [long_read], [(200, 204)], max_indel_size=1000)
    assert R.model(c)[0]["status"] == H.COUNTED
    c = R.case(R.plain(3) + [R.read(150, [(MS, 55), (DE, 901), (MS, 45)])], [(200, 204)], max_indel_size=1000)
    rec = R.model(c)[0]
    assert (rec["status"], rec["reason"]) == (H.DECLINED, H.DECLINE_READ_SPAN)


def test_seeded_window_is_worth_running():
    """what tests/test_region_haplotypes.py asks of its chain case, checked here on the CPU: at least half of the regions counted with two
    or more selected haplotypes, none declined"""
    c, intake, anchor, regions, recs = R.seeded_window_model()
    assert len(regions) >= 20
    assert sum(1 for r in recs if r["status"] == H.COUNTED and len(r["haps"]) >= 2) * 2 >= len(recs)
    assert not any(r["status"] == H.DECLINED for r in recs)
