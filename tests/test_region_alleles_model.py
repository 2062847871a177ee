"""The loop model of processSelectedHaplotypes, discoverIndelsAndMismatches and processDiscoveredIndelsAndMismatches
(tests/alleles_model.py) reproduces what the reference's IndelBuffer and CandidateSnvBuffer held for every recorded region
(tests/golden/region_alleles/, made by tools/golden/make_region_alleles_golden.py); the recorded file exercises every rule the model
has; the bound functions and the record layout of sk_region_alleles.  No device."""
import ctypes as C

import pytest

from tests import alleles_model as A
from tests import haplotype_model as H
from tests import intake_model as M


def _hap_records(sc, ploidy):
    regions = [(g["begin"], g["end"]) for g in sc["regions"] if g["ploidy"] == ploidy]
    return H.region_haplotypes(sc["ref"], sc["ref_offset"], sc["reads"], sc["low"], sc["fwd"], regions, sc["buf_begin"], sc["buf_end"], ploidy, sc["max_indel_size"])


@pytest.mark.parametrize("name", [s["name"] for s in A.golden()])
def test_model_reproduces_the_recorded_scene(built, name):
    sc = next(s for s in A.golden() if s["name"] == name)
    for ploidy in (1, 2):
        recorded = [g for g in sc["regions"] if g["ploidy"] == ploidy]
        for g, hap in zip(recorded, _hap_records(sc, ploidy)):
            what = "%s [%d, %d) ploidy %d prev_end %d" % (name, g["begin"], g["end"], ploidy, g["prev_end"])
            assert hap["status"] == (H.COUNTED if g["counted"] else hap["status"]) and g["counted"] == 1, what
            assert [dict(seq=h["seq"], support=h["support"]) for h in hap["haps"]] == g["selected"], what
            rec = A.process_selected_haplotypes(sc["ref"], sc["ref_offset"], g["begin"], g["end"], g["prev_end"], sc["max_indel_size"], 1024, hap)
            assert rec["status"] == H.COUNTED and rec["prev_end"] == g["prev_end"], what
            keys, snvs = A.replay(g["begin"], rec, hap)
            assert keys == g["keys"], what
            assert snvs == g["snvs"], what
            # the records' own consistency: a first record carries the sums, a repeat names it
            for i, r in enumerate(rec["alleles"]):
                if r["same_as"] >= 0:
                    first = rec["alleles"][r["same_as"]]
                    assert r["same_as"] < i and first["same_as"] == -1 and (first["pos"], first["type"], first["del_len"], first["ins"]) == (r["pos"], r["type"], r["del_len"], r["ins"])
                    assert (r["id_sum"], r["ratio_sum"]) == (0, 0)
                assert r["to_indel_buffer"] == (0 if rec["do_not_add_mismatches"] and r["type"] == A.MISMATCH else 1)


def test_the_recorded_vectors_exercise_every_rule(built):
    counts = A.rule_counts(A.golden())
    assert set(counts) == set(A.RULES)
    for rule in A.RULES:
        assert counts[rule] >= 1, "no recorded region exercises %s: %r" % (rule, counts)


def test_walk_by_hand(built):
    #            100       110
    ref = "GGTCAAAAAATCGGTACGTTAGCATGCA"
    # an insertion of A in the run 104..109 seen in the region [107, 112): shifted to 104; kept from prev_end 104, dropped from 105
    hap = ref[7:10] + "A" + ref[10:12]
    score, keys, n = A.discover_indels_and_mismatches(ref, 100, 107, 112, 104, 49, hap)
    assert (keys, n) == ([(104, A.INDEL, 0, "A")], 1)
    assert A.discover_indels_and_mismatches(ref, 100, 107, 112, 105, 49, hap)[1:] == ([], 0)
    # a deletion of two of them, and a mismatch at 111 that a previous region ending at 112 has taken
    hap = ref[7:8] + ref[10:11] + "A"
    assert A.discover_indels_and_mismatches(ref, 100, 107, 112, -1, 49, hap)[1:] == ([(104, A.INDEL, 2, ""), (111, A.MISMATCH, 1, "A")], 1)
    assert A.discover_indels_and_mismatches(ref, 100, 107, 112, 112, 49, hap)[1:] == ([], 0)
    assert A.discover_indels_and_mismatches(ref, 100, 107, 112, -1, 1, hap)[1:] == ([(111, A.MISMATCH, 1, "A")], 0)  # above max_indel_size
    # an all-N insertion at the start of an all-N reference: the reference's loop would not end
    with pytest.raises(A.Declined) as e:
        A.discover_indels_and_mismatches("NNNNNNNN", 100, 100, 104, -1, 49, "NNNNNN")
    assert e.value.reason == A.DECLINE_LEFT_SHIFT


def test_sums_and_declines_by_hand(built):
    ref = "GGTCAAAAAATCGGTACGTTAGCATGCA"
    seg = ref[7:12]
    mk = lambda seq, n: dict(seq=seq, count=n, is_reference=int(seq == seg), support=list(range(n)))
    # both alternates carry the deletion of two A: ids 1 + 2, ratios 3/7 + 4/7 added in float32
    hap = dict(status=H.COUNTED, reason=0, n_reads_aligned=7, haps=[mk(ref[7:8] + ref[10:12], 4), mk(ref[7:8] + ref[10:11] + "A", 3)])
    rec = A.process_selected_haplotypes(ref, 100, 107, 112, -1, 49, 1024, hap)
    import numpy as np
    f = np.float32
    assert [(r["pos"], r["type"], r["same_as"], r["id_sum"]) for r in rec["alleles"]] == [(104, A.INDEL, -1, 3), (104, A.INDEL, 0, 0), (111, A.MISMATCH, -1, 2)]
    assert rec["alleles"][0]["ratio_sum"] == A.float_bits(f(f(4) / f(7)) + f(f(3) / f(7))) and rec["alleles"][2]["ratio_sum"] == A.float_bits(f(3) / f(7))
    assert (rec["n_alt"], rec["n_indels"], rec["n_distinct_mismatches"], rec["do_not_add_mismatches"], rec["hap_slot"]) == (2, 2, 1, 0, [0, 1])
    # a haplotype above max_hap_len; statuses pass through; only the reference selected
    assert A.process_selected_haplotypes(ref, 100, 107, 112, -1, 49, 3, hap)["status"] == H.COUNTED
    rec = A.process_selected_haplotypes(ref, 100, 107, 112, -1, 49, 2, hap)
    assert (rec["status"], rec["reason"], rec["alleles"]) == (H.DECLINED, A.DECLINE_HAP_LEN, [])
    for status in (H.BYPASSED, H.NO_READS, H.TOO_FEW_COVERING, H.DECLINED):
        rec = A.process_selected_haplotypes(ref, 100, 107, 112, 5, 49, 1024, dict(status=status, reason=2 if status == H.DECLINED else 0, n_reads_aligned=0, haps=[]))
        assert (rec["status"], rec["reason"], rec["prev_end"], rec["alleles"]) == (status, 2 if status == H.DECLINED else 0, 5, [])
    rec = A.process_selected_haplotypes(ref, 100, 107, 112, -1, 49, 1024, dict(status=H.COUNTED, reason=0, n_reads_aligned=5, haps=[mk(seg, 5)]))
    assert (rec["status"], rec["n_alt"], rec["alleles"], rec["do_not_add_mismatches"]) == (H.COUNTED, 0, [], 1)
    # prev_end advances whatever became of a region
    recs, prev_end_out = A.region_alleles(ref, 100, [(102, 104), (107, 112), (115, 118)], [dict(status=H.NO_READS, reason=0, n_reads_aligned=0, haps=[]), hap,
                                                                                            dict(status=H.BYPASSED, reason=0, n_reads_aligned=0, haps=[])], prev_end_in=-1)
    assert [r["prev_end"] for r in recs] == [-1, 104, 112] and prev_end_out == 118
    assert A.region_alleles(ref, 100, [], [], prev_end_in=77) == ([], 77)


def test_id_sum_above_3_declines(built, monkeypatch):
    """the assertion at :752.  No path of the aligner's holds one key twice, so the aligner is replaced: the second alternate's path carries
    the same insertion at two places of a reference of equal bases, and both shift to the one position"""
    ref = "GGTC" + "A" * 12 + "TCGG"
    seg = ref[8:14]  # 108..113, inside the run of A at 104..115
    first, second = "C" + seg[1:], seg + "AA"
    real = A.align

    def fake(haplotype, ref_segment):
        if haplotype == second:
            return 0, 0, [("SEQ_MATCH", 2), ("INSERT", 1), ("SEQ_MATCH", 2), ("INSERT", 1), ("SEQ_MATCH", 2)]
        return real(haplotype, ref_segment)
    monkeypatch.setattr(A, "align", fake)
    mk = lambda seq, n: dict(seq=seq, count=n, is_reference=0, support=list(range(n)))
    hap = dict(status=H.COUNTED, reason=0, n_reads_aligned=8, haps=[mk(first, 4), mk(second, 4)])
    score, keys, n = A.discover_indels_and_mismatches(ref, 100, 108, 114, -1, 49, second)
    assert (keys, n) == ([(104, A.INDEL, 0, "A")] * 2, 2)  # haplotype id 2, twice: 4
    rec = A.process_selected_haplotypes(ref, 100, 108, 114, -1, 49, 1024, hap)
    assert (rec["status"], rec["reason"], rec["alleles"], rec["n_alt"]) == (H.DECLINED, A.DECLINE_ID_SUM, [], 0)
    # as the first alternate the same path gives 1 + 1 = 2, which the reference accepts
    hap = dict(status=H.COUNTED, reason=0, n_reads_aligned=8, haps=[mk(second, 4), mk(first, 4)])
    rec = A.process_selected_haplotypes(ref, 100, 108, 114, -1, 49, 1024, hap)
    assert rec["status"] == H.COUNTED and [(r["same_as"], r["id_sum"]) for r in rec["alleles"][:2]] == [(-1, 2), (0, 0)]


def test_bounds_scratch_and_record_layout(built):
    """host arithmetic: works without a device"""
    from strelka_amd import capi
    L = capi.lib()
    assert L.sk_region_alleles_allele_bound(7, 1024) == 7 * 2 * (250 + 1024) and L.sk_region_alleles_insert_bound(7, 1024) == 7 * 2 * 1024
    assert capi.region_alleles_bounds(3, 1) == (3 * 2 * 251, 6) and capi.region_alleles_bounds(0, 64) == (0, 0)
    for n, m in ((-1, 64), (1, 0), (1, 1025), (1, -5)):
        assert L.sk_region_alleles_allele_bound(n, m) == -1 and L.sk_region_alleles_insert_bound(n, m) == -1
    assert L.sk_region_alleles_scratch_bytes(-1, 64) == 0 and L.sk_region_alleles_scratch_bytes(1, 0) == 0 and L.sk_region_alleles_scratch_bytes(1, 1025) == 0
    small, large = L.sk_region_alleles_scratch_bytes(1, 64), L.sk_region_alleles_scratch_bytes(65, 1024)
    # the records before they are placed and the aligner's back-pointers are in it
    assert small >= 2 * (250 + 64) * 56 + 2 * (64 + 250) * 64 and large >= 65 * (2 * (250 + 1024) * 56 + 2 * 16 * (250 + 64) * 64)
    assert L.sk_region_alleles_scratch_bytes(0, 64) > 0
    assert C.sizeof(capi.RegionAllele) == capi.REGION_ALLELE_DTYPE.itemsize == 56 and C.sizeof(capi.RegionAllelesRec) == capi.REGION_ALLELES_DTYPE.itemsize == 72
    for st, dt in ((capi.RegionAllele, capi.REGION_ALLELE_DTYPE), (capi.RegionAllelesRec, capi.REGION_ALLELES_DTYPE)):
        assert [(n, getattr(st, n).offset) for n, _ in st._fields_] == [(n, dt.fields[n][1]) for n in dt.names]
    assert (capi.ALLELE_DECLINE_BEGIN_POS, capi.ALLELE_DECLINE_LEFT_SHIFT, capi.ALLELE_DECLINE_ID_SUM, capi.ALLELE_DECLINE_HAP_LEN) == \
        (A.DECLINE_BEGIN_POS, A.DECLINE_LEFT_SHIFT, A.DECLINE_ID_SUM, A.DECLINE_HAP_LEN)
    assert M.INDEL_INDEL == capi.INDEL["INDEL"] and A.MISMATCH == capi.INDEL["MISMATCH"]
