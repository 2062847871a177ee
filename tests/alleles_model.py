"""Loop-by-loop model of what an active region does once its haplotypes are selected: ActiveRegionProcessor::processSelectedHaplotypes
(L/starling_common/ActiveRegionProcessor.cpp:518-571), discoverIndelsAndMismatches (:573-707) and
processDiscoveredIndelsAndMismatches (:709-757), over the records of tests/haplotype_model.py.  The alignment is the oracle's restatement
of GlobalAligner<int>::align (oracle.pyoracle.global_align) with the detector's scores.

The IndelBuffer and the CandidateSnvBuffer are a region's own and start empty (`replay` builds them from the records, for comparison with
what the reference's buffers held).  Imports neither the product nor a device."""
import functools
import json
import os
import re

import numpy as np

from oracle import pyoracle
from tests import haplotype_model as H
from tests import intake_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "region_alleles", "region_alleles_golden.json")

MAX_NUM_MISMATCHES_TO_ADD_TO_INDEL_BUFFER = 10  # ActiveRegionProcessor.hh:67
MAX_REF_SPAN = H.MAX_REF_SPAN_TO_BYPASS_ASSEMBLY
INDEL, MISMATCH = M.INDEL_INDEL, 2  # INDEL::INDEL, INDEL::MISMATCH (SK_INDEL_*)
DECLINE_BEGIN_POS, DECLINE_LEFT_SHIFT, DECLINE_ID_SUM, DECLINE_HAP_LEN = 4, 5, 6, 7  # SK_ALLELE_DECLINE_*

_CIGAR = {"=": "SEQ_MATCH", "X": "SEQ_MISMATCH", "I": "INSERT", "D": "DELETE", "S": "SOFT_CLIP"}


class Declined(Exception):
    def __init__(self, reason):
        Exception.__init__(self, reason)
        self.reason = reason


def float_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


@functools.lru_cache(maxsize=None)
def align(haplotype, ref_segment):
    """_aligner.align (:591) -> (score, beginPos, [(segment type, length)])"""
    score, begin_pos, cigar = pyoracle.global_align(haplotype, ref_segment, pyoracle.align_scores())
    return score, begin_pos, [(_CIGAR[t], int(n)) for n, t in re.findall(r"(\d+)(.)", cigar)]


def discover_indels_and_mismatches(ref, ref_offset, begin, end, prev_end, max_indel_size, haplotype, trace=None):
    """:573-707 -> (score, [(pos, type, deletionLength, insertSequence)], numIndels); Declined where the reference asserts (:596-599) or its
    left-shift loop would not end.  trace: a list that receives what became of every indel segment and skipped mismatch (for counting the
    rules a set of vectors exercises)"""
    note = (lambda **kw: trace.append(kw)) if trace is not None else (lambda **kw: None)
    get_base = lambda p: M.ref_char(ref, ref_offset, p)
    ref_segment = "".join(get_base(p) for p in range(begin, end))
    score, begin_pos, path = align(haplotype, ref_segment)
    if begin_pos > 0:
        raise Declined(DECLINE_BEGIN_POS)
    keys = []
    reference_pos, hap_off, num_indels = begin, 0, 0
    if path and path[0][0] == "INSERT":
        note(kind="edge_insertion")
    for seg_type, length in path:
        if seg_type == "SEQ_MATCH":
            reference_pos += length
            hap_off += length
        elif seg_type == "SEQ_MISMATCH":
            for _ in range(length):
                if reference_pos >= prev_end:  # :619
                    keys.append((reference_pos, MISMATCH, 1, haplotype[hap_off]))
                else:
                    note(kind="mismatch_skipped", pos=reference_pos)
                reference_pos += 1
                hap_off += 1
        elif seg_type == "INSERT":
            if length <= max_indel_size:
                insert_pos = reference_pos
                insert_seq = haplotype[hap_off:hap_off + length]
                prev_base = get_base(insert_pos - 1)
                while insert_seq[-1] == prev_base:  # :645-653
                    insert_seq = prev_base + insert_seq[:-1]
                    insert_pos -= 1
                    prev_base = get_base(insert_pos - 1)
                    if insert_pos < ref_offset - length:  # all N from here on: the reference would not stop
                        raise Declined(DECLINE_LEFT_SHIFT)
                kept = prev_base != "N" and insert_pos >= prev_end and insert_pos < end  # :657
                if kept:
                    keys.append((insert_pos, INDEL, 0, insert_seq))
                    num_indels += 1
                note(kind="ins", length=length, pos=insert_pos, shift=reference_pos - insert_pos, kept=kept, next_to_n=prev_base == "N")
            else:
                note(kind="ins", length=length, too_long=True, kept=False)
            hap_off += length
        elif seg_type == "DELETE":
            if length <= max_indel_size:
                delete_pos = reference_pos
                prev_base = get_base(delete_pos - 1)
                last_deletion_base = get_base(delete_pos + length - 1)
                while last_deletion_base == prev_base:  # :678-684
                    delete_pos -= 1
                    last_deletion_base = get_base(delete_pos + length - 1)
                    prev_base = get_base(delete_pos - 1)
                    if delete_pos < ref_offset - length:
                        raise Declined(DECLINE_LEFT_SHIFT)
                kept = prev_base != "N" and delete_pos >= prev_end and delete_pos < end  # :688
                if kept:
                    keys.append((delete_pos, INDEL, length, ""))
                    num_indels += 1
                note(kind="del", length=length, pos=delete_pos, shift=reference_pos - delete_pos, kept=kept, next_to_n=prev_base == "N")
            else:
                note(kind="del", length=length, too_long=True, kept=False)
            reference_pos += length
        else:  # SOFT_CLIP :698-702
            reference_pos += length
    return score, keys, num_indels


def _passed(status, reason, prev_end):
    return dict(status=status, reason=reason, prev_end=prev_end, n_alt=0, n_indels=0, n_distinct_mismatches=0, do_not_add_mismatches=0, score=[], hap_slot=[],
                alleles=[])


def process_selected_haplotypes(ref, ref_offset, begin, end, prev_end, max_indel_size, max_hap_len, hap_rec, trace=None):
    """:518-571 with :709-757 for one region -> the record capi.region_allele_records gives"""
    if hap_rec["status"] != H.COUNTED or not hap_rec["haps"]:
        return _passed(hap_rec["status"], hap_rec["reason"], prev_end)
    alts = [k for k, h in enumerate(hap_rec["haps"]) if h["seq"] != "".join(M.ref_char(ref, ref_offset, p) for p in range(begin, end))]  # :529
    assert len(alts) <= 2 and all(not hap_rec["haps"][k]["is_reference"] for k in alts)
    if any(len(hap_rec["haps"][k]["seq"]) > max_hap_len for k in alts):
        return _passed(H.DECLINED, DECLINE_HAP_LEN, prev_end)
    discovered, scores = [], []
    is_any_indel, mismatch_set, n_indels = False, set(), 0
    try:
        for k in alts:
            score, keys, num_indels = discover_indels_and_mismatches(ref, ref_offset, begin, end, prev_end, max_indel_size, hap_rec["haps"][k]["seq"], trace)
            for key in keys:
                if key[1] == MISMATCH:
                    mismatch_set.add(key)
                else:
                    is_any_indel = True
            discovered.append(keys)
            scores.append(score)
            n_indels += num_indels
    except Declined as d:
        return _passed(H.DECLINED, d.reason, prev_end)
    do_not_add = (not is_any_indel) or len(mismatch_set) > MAX_NUM_MISMATCHES_TO_ADD_TO_INDEL_BUFFER  # :553-560
    records, first_of = [], {}
    for haplotype_id, (k, keys) in enumerate(zip(alts, discovered), 1):  # :562-570
        hap = hap_rec["haps"][k]
        ratio = np.float32(len(hap["support"])) / np.float32(hap_rec["n_reads_aligned"])  # :719
        for key in keys:
            rec = dict(pos=key[0], type=key[1], del_len=key[2], ins=key[3], hap_slot=k, haplotype_id=haplotype_id, ratio=float_bits(ratio),
                       to_indel_buffer=0 if (do_not_add and key[1] == MISMATCH) else 1, same_as=first_of.get(key, -1), id_sum=0, ratio_sum=float_bits(0.0))
            first_of.setdefault(key, len(records))
            records.append(rec)
            if not rec["to_indel_buffer"]:
                continue  # :731
            first = records[first_of[key]]
            first["id_sum"] += haplotype_id  # :750
            first["_ratio_sum"] = np.float32(first.get("_ratio_sum", np.float32(0.0)) + ratio)  # :755
            first["ratio_sum"] = float_bits(first["_ratio_sum"])
    if any(r["id_sum"] > 3 for r in records):  # the assertion at :752
        return _passed(H.DECLINED, DECLINE_ID_SUM, prev_end)
    for r in records:
        r.pop("_ratio_sum", None)
    return dict(status=H.COUNTED, reason=0, prev_end=prev_end, n_alt=len(alts), n_indels=n_indels, n_distinct_mismatches=len(mismatch_set),
                do_not_add_mismatches=int(do_not_add), score=scores, hap_slot=alts, alleles=records)


def region_alleles(ref, ref_offset, regions, hap_recs, max_indel_size=M.MAX_INDEL_SIZE, max_hap_len=1024, prev_end_in=-1):
    """the whole of sk_region_alleles: regions = [(begin, end)], hap_recs = haplotype_model.region_haplotypes' records -> (records, prev_end_out)"""
    out = []
    prev_end = prev_end_in
    for (begin, end), hap_rec in zip(regions, hap_recs):
        out.append(process_selected_haplotypes(ref, ref_offset, int(begin), int(end), prev_end, max_indel_size, max_hap_len, hap_rec))
        prev_end = int(end)  # ActiveRegionDetector.cpp:248: whatever became of the region
    return out, prev_end


def replay(begin, rec, hap_rec):
    """what a router does with a region's records on empty buffers -> (keys as the golden file lists an IndelBuffer, in IndelKey order; the
    CandidateSnvBuffer's [pos, a, c, g, t, ratio bits])"""
    keys, snvs = {}, {}
    for r in rec["alleles"]:
        ratio = np.array([r["ratio"]], np.uint32).view(np.float32)[0]
        if r["type"] == MISMATCH:  # addCandidateSnv :725-728
            s = snvs.setdefault(r["pos"], dict(A=0, C=0, G=0, T=0, ratio=np.float32(0.0)))
            s[r["ins"]] += r["haplotype_id"]
            s["ratio"] = np.float32(s["ratio"] + ratio)
        if not r["to_indel_buffer"]:
            continue
        k = (r["pos"], r["type"], r["del_len"], r["ins"])
        d = keys.setdefault(k, dict(ids=set(), haplotype_id=0, ratio=np.float32(0.0)))
        d["ids"].update(hap_rec["haps"][r["hap_slot"]]["support"])
        d["haplotype_id"] += r["haplotype_id"]
        d["ratio"] = np.float32(d["ratio"] + ratio)
    order = sorted(keys, key=lambda k: (k[0], k[1], len(k[3]), k[2], k[3].encode()))  # IndelKey::operator< (IndelKey.hh:56-76)
    return ([dict(pos=k[0], type=k[1], del_len=k[2], ins=k[3], active_region_id=begin, haplotype_id=keys[k]["haplotype_id"], ratio=float_bits(keys[k]["ratio"]),
                  ids=sorted(keys[k]["ids"])) for k in order],
            [[p, s["A"], s["C"], s["G"], s["T"], float_bits(s["ratio"])] for p, s in sorted(snvs.items())])


@functools.lru_cache(maxsize=None)
def golden():
    """-> [dict(name, ref, ref_offset, reads, low, fwd, max_indel_size, buf_begin, buf_end, regions [recorded dicts])]"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = []
    for sc in doc["scenes"]:
        reads = [dict(code=M.encode(r["seq"]), pos=r["pos"], path=[tuple(s) for s in r["path"]]) for r in sc["reads"]]
        out.append(dict(name=sc["name"], ref=sc["ref"], ref_offset=sc["ref_offset"], reads=reads, low=[r["low_mapq"] for r in sc["reads"]],
                        fwd=[r["is_fwd"] for r in sc["reads"]], max_indel_size=sc["max_indel_size"], buf_begin=sc["buf_begin"], buf_end=sc["buf_end"],
                        regions=sc["regions"]))
    return out


# The rules a set of recorded vectors has to exercise.  Of "left-shifted to end - 1 and to end": an indel the walk meets at reference
# position p <= end is never moved right, so one that ends at `end` was not shifted, and a deletion's start is always below `end` -- there is
# no deletion at `end`; the three rules at the region's end therefore ask for the position and the outcome, not for a shift.  The
# edge insertion has to be kept at the region's first position itself (the path begins with it and nothing moves it).
RULES = ("one_alternate", "two_alternates", "top_not_reference", "only_reference", "same_indel_in_both_alternates", "same_position_different_bases",
         "ten_mismatches_with_an_indel", "eleven_mismatches_with_an_indel", "mismatches_without_indel", "insertion_shifted_to_prev_end",
         "insertion_shifted_below_prev_end", "deletion_shifted_to_prev_end", "deletion_shifted_below_prev_end", "insertion_at_end_minus_1", "insertion_at_end",
         "deletion_at_end_minus_1", "insertion_next_to_n", "deletion_next_to_n", "indel_of_max_indel_size", "indel_above_max_indel_size", "edge_insertion",
         "snv_in_a_shared_base", "ploidy_1", "inexact_ratio_sum")


def rule_counts(scenes):
    """how many recorded regions exercise each rule of RULES (the recorded fields, and the model's trace for what a region dropped)"""
    n = dict.fromkeys(RULES, 0)
    for sc in scenes:
        for gi, g in enumerate(sc["regions"]):
            if not g["counted"]:
                continue
            ref_segment = "".join(M.ref_char(sc["ref"], sc["ref_offset"], p) for p in range(g["begin"], g["end"]))
            alts = [h for h in g["selected"] if h["seq"] != ref_segment]
            hap_rec = dict(status=H.COUNTED, reason=0, n_reads_aligned=g["n_reads_aligned"],
                           haps=[dict(seq=h["seq"], support=h["support"], is_reference=int(h["seq"] == ref_segment)) for h in g["selected"]])
            trace = []
            process_selected_haplotypes(sc["ref"], sc["ref_offset"], g["begin"], g["end"], g["prev_end"], sc["max_indel_size"], 1024, hap_rec, trace)
            indel_keys = [k for k in g["keys"] if k["type"] == INDEL]
            mismatch_keys = [k for k in g["keys"] if k["type"] == MISMATCH]
            n_snv = sum(1 for s in g["snvs"] for x in s[1:5] if x)
            n["one_alternate"] += len(alts) == 1
            n["two_alternates"] += len(alts) == 2
            n["top_not_reference"] += bool(g["selected"]) and g["selected"][0]["seq"] != ref_segment and len(g["selected"]) > len(alts)
            n["only_reference"] += bool(g["selected"]) and not alts
            n["same_indel_in_both_alternates"] += any(k["haplotype_id"] == 3 for k in indel_keys)
            n["same_position_different_bases"] += any(sum(1 for x in s[1:5] if x) == 2 for s in g["snvs"])
            n["ten_mismatches_with_an_indel"] += n_snv == 10 and bool(indel_keys) and len(mismatch_keys) == 10
            n["eleven_mismatches_with_an_indel"] += n_snv == 11 and bool(indel_keys) and not mismatch_keys
            n["mismatches_without_indel"] += n_snv > 0 and not g["keys"]
            for kind in ("ins", "del"):
                name = "insertion" if kind == "ins" else "deletion"
                t = [x for x in trace if x["kind"] == kind and not x.get("too_long")]
                n[name + "_shifted_to_prev_end"] += any(x["kept"] and x["shift"] > 0 and x["pos"] == g["prev_end"] for x in t)
                n[name + "_shifted_below_prev_end"] += any(not x["kept"] and x["shift"] > 0 and x["pos"] == g["prev_end"] - 1 for x in t)
                n[name + "_at_end_minus_1"] += any(x["kept"] and x["pos"] == g["end"] - 1 for x in t)
                n[name + "_next_to_n"] += any(not x["kept"] and x["next_to_n"] and x["shift"] > 0 for x in t)
            n["insertion_at_end"] += any(x["kind"] == "ins" and not x.get("too_long") and not x["kept"] and x["pos"] == g["end"] for x in trace)
            n["indel_of_max_indel_size"] += any(x["kind"] in ("ins", "del") and x["kept"] and x["length"] == sc["max_indel_size"] for x in trace)
            n["indel_above_max_indel_size"] += any(x.get("too_long") and x["length"] == sc["max_indel_size"] + 1 for x in trace)
            n["edge_insertion"] += any(x["kind"] == "edge_insertion" for x in trace) and \
                any(x["kind"] == "ins" and x["kept"] and x["pos"] == g["begin"] and x["shift"] == 0 for x in trace)
            prev = sc["regions"][gi - 2] if gi >= 2 else None  # (every region is recorded at ploidy 1 and 2)
            n["snv_in_a_shared_base"] += bool(prev) and prev["ploidy"] == g["ploidy"] and g["begin"] == prev["end"] - 1 and g["prev_end"] == prev["end"] and \
                any(s[0] == g["begin"] for s in prev["snvs"]) and any(x["kind"] == "mismatch_skipped" and x["pos"] == g["begin"] for x in trace)
            n["ploidy_1"] += g["ploidy"] == 1 and bool(g["keys"] or g["snvs"])
            n["inexact_ratio_sum"] += g["n_reads_aligned"] == 7 and sorted(len(h["support"]) for h in alts) == [3, 4] and any(k["haplotype_id"] == 3 for k in g["keys"])
    return {k: int(v) for k, v in n.items()}
