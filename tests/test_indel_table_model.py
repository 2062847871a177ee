"""The indel-table model (tests/indel_table_model.py) against what the reference's IndelBuffer held
(tests/golden/indel_table/indel_table_golden.json, recorded by tools/golden/indel_buffer_driver.cpp): every key, id set, report field,
doNotGenotype, activeRegionId, haplotypeId, ratio bits and bypass mark of every scene.  Rules 8 and 9 -- a pair the assembler would
take, and refused input -- cannot be recorded from the reference and are hand cases here.  Needs no device."""
import numpy as np
import pytest

from tests import haplotype_model as H
from tests import indel_table_cases as K
from tests import indel_table_model as T

SCENES = [s["name"] for s in T.golden()]


@pytest.fixture(scope="module")
def modelled():
    """every recorded scene through the model, once"""
    out = {}
    for sc in T.golden():
        samples, regions = T.scene_samples(sc)
        keys, totals = T.indel_table(sc["ref"], sc["ref_offset"], samples, regions, sc["prev_end_in"])
        out[sc["name"]] = (samples, regions, keys, totals, sc["ref"], sc["ref_offset"])
    return out


@pytest.mark.parametrize("name", SCENES)
def test_model_equals_the_reference_field_for_field(name, modelled):
    sc = next(s for s in T.golden() if s["name"] == name)
    samples, regions, keys, totals = modelled[name][:4]
    assert sc["assembled"] == 0                                 # the reference never reached the assembler
    assert not any(k["flags"] & T.AR_PENDING for k in keys)     # and the model has no pair whose outcome is not known
    assert T.as_recorded(keys) == sc["keys"]
    assert totals == [len(keys), sum(len(x) for k in keys for d in k["samples"] for x in d["ids"]), sum(len(k["ins"]) for k in keys), 0]


def test_every_rule_is_exercised_by_the_recorded_scenes(modelled):
    counts = T.rule_counts([(v[0], v[1], v[2], v[4], v[5]) for v in modelled.values()])
    assert set(counts) == set(T.RULES)
    assert all(n > 0 for n in counts.values()), counts
    assert len(T.golden()) >= 25 and sum(len(s["samples"]) > 1 for s in T.golden()) >= 4


def test_key_order_is_ascii_and_insert_length_comes_before_delete_length():
    reads = ["GATTACAT", "GATTNCAT", "GATTGCAT"]
    s = K.sample(reads, [K.obs(0, 210, ins=(3, 2)), K.obs(1, 210, ins=(3, 2)), K.obs(2, 210, ins=(3, 2)),    # TA, TN, TG
                         K.obs(0, 210, del_len=2, ins=(0, 1)), K.obs(1, 210, del_len=1, ins=(0, 2)),        # (ins 1, del 2), (ins 2, del 1)
                         K.obs(0, 210, K.BP_RIGHT), K.obs(0, 210, K.BP_LEFT, ins=(0, 3)), K.obs(1, 210, K.BP_LEFT, ins=(2, 4))])
    keys, totals = T.indel_table(K.REF, K.REF_OFFSET, [s], [])
    assert [(k["type"], k["del_len"], k["ins"]) for k in keys] == [(K.INDEL, 2, "G"), (K.INDEL, 0, "TA"), (K.INDEL, 0, "TG"), (K.INDEL, 0, "TN"), (K.INDEL, 1, "GA"),
                                                                  (K.BP_LEFT, 0, ""), (K.BP_RIGHT, 0, "")]
    assert [k["n_bp_obs"] for k in keys] == [0, 0, 0, 0, 0, 2, 1] and keys[5]["samples"][0]["ids"][T.TIER1] == [0, 1]
    assert [bool(k["flags"] & T.DO_NOT_GENOTYPE) for k in keys] == [True, False, False, False, True, True, True]


def _pending_case(status, allele_status=H.COUNTED):
    reads = ["ACGTACGT"] * 4
    s0 = K.sample(reads, [K.obs(0, 195, del_len=1), K.obs(1, 205, del_len=1), K.obs(2, 212, del_len=1), K.obs(3, 230, del_len=1)],
                  hap=[K.hap_rec(H.COUNTED, [[0], [1, 2]]), K.hap_rec(status, [])],
                  alleles=[K.allele_rec([K.allele(180, del_len=3)]), K.allele_rec([], status=allele_status if status == H.COUNTED else status)])
    return s0, [(170, 190), (200, 210)]


@pytest.mark.parametrize("status", [H.NO_READS, H.TOO_FEW_COVERING, H.DECLINED, "alleles_declined"])
def test_rule_8_a_pending_pair_writes_nothing_and_flags_from_prev_end(status):
    s0, regions = _pending_case(*((H.COUNTED, H.DECLINED) if status == "alleles_declined" else (status,)))
    keys, totals = T.indel_table(K.REF, K.REF_OFFSET, [s0], regions, prev_end_in=-1)
    by_pos = {k["pos"]: k for k in keys}
    # the second region's prev_end is 190: keys in [190, 210) are flagged, the one at 212 and the first region's at 180 are not
    assert {p: bool(k["flags"] & T.AR_PENDING) for p, k in by_pos.items()} == {180: False, 195: True, 205: True, 212: False, 230: False}
    assert totals[3] == 1 and by_pos[205]["active_region_id"] == -1 and by_pos[205]["samples"][0]["is_haplotyping_bypassed"] == 0
    assert by_pos[180]["active_region_id"] == 170 and by_pos[180]["samples"][0]["haplotype_id"] == 1


def test_rule_8_a_negative_prev_end_counts_as_zero():
    s0, regions = _pending_case(H.NO_READS)
    s0["hap"], s0["alleles"] = s0["hap"][1:], s0["alleles"][1:]
    keys, totals = T.indel_table(K.REF, K.REF_OFFSET, [s0], regions[1:], prev_end_in=-1)
    assert [bool(k["flags"] & T.AR_PENDING) for k in keys] == [True, True, False, False] and totals[3] == 1  # min(200, max(-1, 0)) = 0


def test_rule_9_refusals():
    ok = K.deletions_case(2)
    T.indel_table(K.REF, K.REF_OFFSET, [ok], [])
    with pytest.raises(T.Refused, match="SK_MAX_SAMPLES"):
        T.indel_table(K.REF, K.REF_OFFSET, [ok] * 9, [])
    with pytest.raises(T.Refused, match="SK_MAX_SAMPLES"):
        T.indel_table(K.REF, K.REF_OFFSET, [], [])
    with pytest.raises(T.Refused, match="iat above 2"):
        T.indel_table(K.REF, K.REF_OFFSET, [K.deletions_case(2, iat=[0, 3])], [])
    with pytest.raises(T.Refused, match="outside its read"):
        T.indel_table(K.REF, K.REF_OFFSET, [K.sample(["ACGT"], [K.obs(0, 200, ins=(2, 3))])], [])
    with pytest.raises(T.Refused, match="outside the sample"):
        T.indel_table(K.REF, K.REF_OFFSET, [K.sample(["ACGT"], [K.obs(1, 200, del_len=1)])], [])
    bad = K.sample(["ACGT"] * 3, [], hap=[K.hap_rec(H.COUNTED, [[0], [1, 7]])], alleles=[K.allele_rec([K.allele(200, del_len=1)])])
    with pytest.raises(T.Refused, match="support list"):
        T.indel_table(K.REF, K.REF_OFFSET, [bad], [(195, 205)])
    bad = K.sample(["ACGT"] * 3, [], hap=[K.hap_rec(H.COUNTED, [[0], [1, 2]])], alleles=[K.allele_rec([K.allele(200, del_len=1, hap_slot=2)])])
    with pytest.raises(T.Refused, match="did not select"):
        T.indel_table(K.REF, K.REF_OFFSET, [bad], [(195, 205)])


def test_ratio_sums_are_ordered_float_additions():
    third, tenth = np.float32(1) / np.float32(3), np.float32(0.1)
    s = K.sample(["ACGT"] * 6, [], hap=[K.hap_rec(H.COUNTED, [[0], [1, 2], [3, 4, 5]])],
                 alleles=[K.allele_rec([K.allele(200, del_len=1, hap_slot=1, haplotype_id=1, ratio=third), K.allele(200, del_len=1, hap_slot=2, haplotype_id=2, ratio=tenth)])])
    keys, _ = T.indel_table(K.REF, K.REF_OFFSET, [s], [(195, 205)])
    d = keys[0]["samples"][0]
    assert (d["haplotype_id"], d["ratio"]) == (3, T.float_bits(np.float32(np.float32(0.0) + third) + tenth)) and d["ids"][T.TIER1] == [1, 2, 3, 4, 5]
