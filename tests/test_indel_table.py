"""The indel table on the device (sk_indel_table, csrc/indel_table.hip): every field of every key and of every (key, sample) record equals
the loop model (tests/indel_table_model.py, itself pinned to vectors recorded from the reference by tests/test_indel_table_model.py).

The shapes are the smallest at which the kernels can go wrong: the wave edge (63 / 64 / 65 reads on a key), the sort tile of 1 024
expanded records (tile - 1, tile, tile + 1, 3 * tile + 1: one, two and four tiles, so one and two merge passes), keys that tie down to
the last insert byte, eight samples.  No case outside the pending test may produce AR_PENDING."""
import ctypes as C

import numpy as np
import pytest

from strelka_amd import capi
from tests import haplotype_model as H
from tests import indel_table_cases as K
from tests import indel_table_model as T
from tests import test_indel_table_model as TM

pytestmark = pytest.mark.gpu

TILE = 1024  # IT_TILE of csrc/indel_table.hip


def _check_layout(raw, n_samples):
    """the keys' insert bytes and the id lists lie back to back in (key, sample, set) order, totals count them, all padding is zero"""
    at_ins = at_id = 0
    for k, key in enumerate(raw["keys"]):
        assert int(key["ins_off"]) == at_ins
        at_ins += int(key["ins_len"])
        for d in raw["data"][k * n_samples:(k + 1) * n_samples]:
            assert int(d["pad"]) == 0
            for c in range(capi.ITAB_N_SETS):
                assert int(d["off"][c]) == at_id
                ids = raw["id_pool"][at_id:at_id + int(d["count"][c])].tolist()
                assert ids == sorted(set(ids))  # ascending and unique, as std::set<align_id_t> iterates
                at_id += int(d["count"][c])
    assert raw["totals"].tolist()[:3] == [len(raw["keys"]), at_id, at_ins] and len(raw["id_pool"]) == at_id and len(raw["insert_pool"]) == at_ins
    assert len(raw["data"]) == len(raw["keys"]) * n_samples
    # (the key record is 14 words with no hole: pos .. interrupted_hpol_len; the data record's only padding is `pad`)
    assert capi.INDEL_TABLE_KEY_DTYPE.itemsize == 4 * 4 + 8 + 8 * 4


def _table(samples, regions=(), prev_end_in=-1, ref=K.REF, ref_offset=K.REF_OFFSET, pending_allowed=False, dev_samples=None):
    """device against model -> the model's (keys, totals)"""
    capi.init(0)
    want, totals = T.indel_table(ref, ref_offset, samples, list(regions), prev_end_in)
    raw = capi.indel_table(ref, ref_offset, dev_samples or [K.device_sample(s) for s in samples], list(regions), prev_end_in, raw=True)
    _check_layout(raw, len(samples))
    got = capi.indel_table_records(raw["keys"], raw["data"], raw["id_pool"], raw["insert_pool"], len(samples))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    assert raw["totals"].tolist() == totals
    if not pending_allowed:
        assert totals[3] == 0 and not any(k["flags"] & T.AR_PENDING for k in want)
    return want, totals


def test_empty_input_gives_an_empty_table():
    assert _table([K.sample([], [])]) == ([], [0, 0, 0, 0])
    assert _table([K.sample(["ACGT", "ACGT"], [])] * 3) == ([], [0, 0, 0, 0])


def test_one_read_one_key():
    want, totals = _table([K.sample(["ACGTTGCA"], [K.obs(0, 200, ins=(2, 3))], align_id=[41], iat=[2])])
    assert totals == [1, 1, 3, 0] and want[0]["ins"] == "GTT" and want[0]["samples"][0]["ids"] == [[], [], [41], []]


@pytest.mark.parametrize("n_reads", [63, 64, 65])
def test_wave_edge_reads_on_one_key(n_reads):
    ids = [1000 - 3 * r for r in range(n_reads)]  # descending: the sets come out ascending
    want, totals = _table([K.deletions_case(n_reads, align_id=ids, iat=[r % 3 for r in range(n_reads)])])
    assert totals[:2] == [1, n_reads] and sum(len(x) for x in want[0]["samples"][0]["ids"]) == n_reads


def test_one_key_seen_by_eight_samples():
    samples = [K.deletions_case(3 + s, align_id=[100 * s + r for r in range(3 + s)]) for s in range(8)]
    want, totals = _table(samples)
    assert totals[:2] == [1, sum(3 + s for s in range(8))] and [len(d["ids"][0]) for d in want[0]["samples"]] == [3 + s for s in range(8)]


def test_duplicates_within_a_set_are_one_member_and_sets_are_separate():
    # read 1 saw the deletion itself (as noise) and supports the haplotype that has it; read 2 saw it cleanly and supports it too
    s = K.sample(["ACGTACGT"] * 4, [K.obs(1, 200, del_len=2, noise=1), K.obs(2, 200, del_len=2)], align_id=[10, 11, 12, 13],
                 hap=[K.hap_rec(H.COUNTED, [[0], [1, 2, 3]])], alleles=[K.allele_rec([K.allele(200, del_len=2)])])
    want, totals = _table([s], [(195, 205)])
    assert want[0]["samples"][0]["ids"] == [[11, 12, 13], [], [], [11]] and totals[:2] == [1, 4]
    assert (want[0]["active_region_id"], want[0]["samples"][0]["haplotype_id"]) == (195, 1)


def test_key_order():
    TM.test_key_order_is_ascii_and_insert_length_comes_before_delete_length()  # (what the case is expected to give, on the model)
    reads = ["GATTACAT", "GATTNCAT", "GATTGCAT"]
    s = K.sample(reads, [K.obs(0, 210, ins=(3, 2)), K.obs(1, 210, ins=(3, 2)), K.obs(2, 210, ins=(3, 2)), K.obs(0, 210, del_len=2, ins=(0, 1)),
                         K.obs(1, 210, del_len=1, ins=(0, 2)), K.obs(0, 210, K.BP_RIGHT), K.obs(0, 210, K.BP_LEFT, ins=(0, 3)), K.obs(1, 210, K.BP_LEFT, ins=(2, 4))],
                 hap=[K.hap_rec(H.COUNTED, [[0], [1, 2]])], alleles=[K.allele_rec([K.allele(210, K.MISMATCH, 1, "T"), K.allele(209, del_len=1)])])
    want, _ = _table([s], [(205, 215)])
    assert [k["type"] for k in want] == [K.INDEL] + [K.INDEL] * 5 + [K.MISMATCH, K.BP_LEFT, K.BP_RIGHT]
    assert [k["ins"] for k in want[2:5]] == ["TA", "TG", "TN"] and want[7]["n_bp_obs"] == 2


def test_inserts_that_differ_in_the_last_base_only():
    stem = "ACGTACGTACGTACGTACGTACG"
    reads = [stem + b for b in "TNGCA"] + [stem + "C"]
    want, totals = _table([K.sample(reads, [K.obs(r, 222, ins=(0, 24)) for r in range(6)])])
    assert [k["ins"][-1] for k in want] == ["A", "C", "G", "N", "T"] and want[1]["samples"][0]["ids"][0] == [3, 5] and totals[2] == 5 * 24


def _distinct_descending(n):
    """n reads, each with a key of its own, presented in descending key order"""
    return K.sample(["ACGT"] * n, [K.obs(r, 150 + (n - r) // 3, del_len=1 + (n - r) % 3) for r in range(n)])


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_sort_tiles_all_keys_equal(n):
    want, totals = _table([K.deletions_case(n, align_id=[(13 * r) % n for r in range(n)])])  # 13 is coprime to every n here: a permutation
    assert totals[:2] == [1, n] and want[0]["samples"][0]["ids"][0] == list(range(n))


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_sort_tiles_all_keys_distinct_and_descending(n):
    want, totals = _table([_distinct_descending(n)])
    assert totals[:2] == [n, n] and [(k["pos"], k["del_len"]) for k in want] == sorted((k["pos"], k["del_len"]) for k in want)


def test_duplicate_ids_across_a_tile_border():
    n = TILE + 40
    s = K.deletions_case(n, align_id=[r // 2 for r in range(n)])  # every id twice; the sorted run of equal records crosses the border
    want, totals = _table([s])
    assert totals[:2] == [1, n // 2]


@pytest.mark.parametrize("name", TM.SCENES)
def test_recorded_scenes_through_the_chain_of_host_entries(name):
    """the reference's scenes: sk_read_intake -> sk_region_haplotypes -> sk_region_alleles per sample, then sk_indel_table; the table
    against the model and against what the reference's IndelBuffer held"""
    capi.init(0)
    sc = next(s for s in T.golden() if s["name"] == name)
    samples, regions = T.scene_samples(sc)
    opt = capi.intake_options()
    opt.max_indel_size = sc["max_indel_size"]
    dev_samples = []
    for sm in samples:
        intake = capi.read_intake(sc["ref"], sc["ref_offset"], sm["reads"], sm["low"], 0, 0, opt)
        hap = capi.region_haplotypes(sc["ref"], sc["ref_offset"], sm["reads"], sm["low"], sm["fwd"], regions, sm["buf_begin"], sm["buf_end"], sm["ploidy"], intake=intake,
                                     opt=opt, raw=True)
        alleles = capi.region_alleles(sc["ref"], sc["ref_offset"], regions, hap, sc["max_indel_size"], 1024, sc["prev_end_in"], raw=True)
        dev_samples.append(dict(reads=sm["reads"], intake=intake, align_id=sm["align_id"], iat=sm["iat"], haplotypes=hap, alleles=alleles))
    want, _ = _table(samples, regions, sc["prev_end_in"], ref=sc["ref"], ref_offset=sc["ref_offset"], dev_samples=dev_samples)
    assert T.as_recorded(want) == sc["keys"]


def test_report_info_hand_cases():
    # a swap with unequal units (counts stay 0), one with equal units, and the four probed positions of the interrupted homopolymer
    ref = "GCATATATGC" + "TTTTTCTTTTT" + "GACCCCCAG" + "ACGTTTTTTT"
    s = K.sample(["ATGG", "CCAT"], [K.obs(0, 104, del_len=2, ins=(2, 2)), K.obs(0, 104, del_len=4, ins=(0, 2)), K.obs(1, 123, del_len=1),
                                    K.obs(1, 110, ins=(0, 1)), K.obs(1, 121, del_len=7, ins=(3, 1)), K.obs(1, 133, ins=(3, 1))])
    want, _ = _table([s], ref=ref, ref_offset=100)
    by = {(k["pos"], k["del_len"], k["ins"]): k for k in want}
    assert (by[(104, 2, "GG")]["it"], by[(104, 2, "GG")]["repeat_unit_len"], by[(104, 2, "GG")]["ref_repeat_count"]) == (T.IT_SWAP, 0, 0)
    assert by[(104, 4, "AT")]["repeat_unit_len"] == 2 and by[(104, 4, "AT")]["ref_repeat_count"] == 3 and by[(104, 4, "AT")]["indel_repeat_count"] == 2
    assert by[(123, 1, "")]["ref_repeat_count"] == 5 and by[(133, 0, "T")]["indel_repeat_count"] == 8  # the run to ref.end()
    assert by[(110, 0, "C")]["interrupted_hpol_len"] == 10 and by[(121, 7, "T")]["interrupted_hpol_len"] == 10


def test_interrupted_homopolymer_each_probed_position_decides_alone():
    """four deletions; for each, one of pos - 1, pos, right - 1, right alone gives the maximum: leaving any probe out changes a field"""
    ref = "ACGT" * 12 + "CTGAAAATAAAACGT" + "ACGTACG" + "CTGCAAAATAAAAGT" + "ACGTACG" + "GCCCCTCCCCAGTAC" + "ACGTACG" + "GATTTTCTTTTGACA" + "ACGT" * 5
    keys = [(150, 10), (172, 2), (202, 3), (216, 10)]
    probes = [T.interrupted_hpol_probes(ref, 100, (p, K.INDEL, n, "")) for p, n in keys]
    for which, values in zip((2, 3, 0, 1), probes):  # right - 1, right, pos - 1, pos: the run of 4 + 4 around one other base, everything else at most 4
        assert values[which] == 8 and max(values[:which] + values[which + 1:]) <= 4, (which, values)
    want, _ = _table([K.sample(["ACGT"], [K.obs(0, p, del_len=n) for p, n in keys])], ref=ref, ref_offset=100)
    assert [(k["pos"], k["interrupted_hpol_len"]) for k in want] == [(150, 8), (172, 8), (202, 8), (216, 8)]


def test_a_repeat_unit_of_n_before_the_segment():
    """get_base gives N before the segment, so the reference's upstream walk of an all-N unit runs to position 0; the device counts those
    steps without taking them"""
    ref = "NNAC" + "GTCA" * 10
    s = K.sample(["NNAC"], [K.obs(0, 100, ins=(0, 1)), K.obs(0, 100, del_len=1), K.obs(0, 100, ins=(0, 2)), K.obs(0, 103, ins=(0, 1))])
    want, _ = _table([s], ref=ref, ref_offset=100)
    by = {(k["pos"], k["del_len"], k["ins"]): k for k in want}
    assert (by[(100, 0, "N")]["ref_repeat_count"], by[(100, 0, "N")]["indel_repeat_count"]) == (102, 103)  # 100 steps before the segment, 2 in it
    assert (by[(100, 1, "")]["ref_repeat_count"], by[(100, 1, "")]["indel_repeat_count"]) == (102, 101)
    assert (by[(100, 0, "NN")]["repeat_unit_len"], by[(100, 0, "NN")]["indel_repeat_count"]) == (1, 104)
    assert by[(103, 0, "N")]["indel_repeat_count"] == 1  # an N unit away from any N: nothing upstream


def test_ratio_sum_follows_region_order_whatever_the_order_of_the_records_in_memory():
    """three regions hand the same key back with ratios whose float sum depends on the order: (1/3 + 1/7) + 3/11 is one bit above
    (1/3 + 3/11) + 1/7.  The second and third regions' records change places in the alleles array; the sum stays the region order's"""
    f = np.float32
    ratios = [f(1) / f(3), f(1) / f(7), f(3) / f(11)]
    assert T.float_bits(f(f(ratios[0] + ratios[1]) + ratios[2])) != T.float_bits(f(f(ratios[0] + ratios[2]) + ratios[1]))
    s = K.sample(["ACGT"] * 3, [], hap=[K.hap_rec(H.COUNTED, [[0], [1, 2]])] * 3, alleles=[K.allele_rec([K.allele(200, del_len=1, ratio=r)]) for r in ratios])
    d = K.device_sample(s)
    al, recs = d["alleles"]["alleles"], d["alleles"]["recs"]
    al[[1, 2]] = al[[2, 1]]
    recs[1]["allele_off"], recs[2]["allele_off"] = 2, 1
    want, _ = _table([s], [(190, 195), (195, 205), (205, 210)], dev_samples=[d])
    assert want[0]["samples"][0]["ratio"] == T.float_bits(f(f(ratios[0] + ratios[1]) + ratios[2])) and want[0]["samples"][0]["haplotype_id"] == 3


def test_bypassed_regions_overlap_and_the_last_writer_wins():
    reads = ["ACGTACGT"] * 3
    s0 = K.sample(reads, [K.obs(0, 204, del_len=1), K.obs(1, 208, del_len=1), K.obs(2, 208, K.BP_LEFT)], hap=[K.hap_rec(H.BYPASSED), K.hap_rec(H.BYPASSED)],
                  alleles=[K.allele_rec(status=H.BYPASSED), K.allele_rec(status=H.BYPASSED)])
    s1 = K.sample(reads, [], hap=[K.hap_rec(H.BYPASSED), K.hap_rec(H.COUNTED, [[0, 1, 2]])], alleles=[K.allele_rec(status=H.BYPASSED), K.allele_rec()])
    want, _ = _table([s0, s1], [(200, 209), (208, 215)])
    by = {(k["pos"], k["type"]): k for k in want}
    assert by[(204, K.INDEL)]["active_region_id"] == 200 and by[(208, K.INDEL)]["active_region_id"] == 208 and by[(208, K.BP_LEFT)]["active_region_id"] == -1
    assert [d["is_haplotyping_bypassed"] for d in by[(208, K.INDEL)]["samples"]] == [1, 1] and by[(208, K.BP_LEFT)]["samples"][0]["is_haplotyping_bypassed"] == 0


@pytest.mark.parametrize("bypassed_sample", [0, 1])
def test_a_key_discovered_after_a_sample_bypassed_is_not_marked(bypassed_sample):
    reads = ["ACGTACGT"] * 4
    counted = K.sample(reads, [], hap=[K.hap_rec(H.COUNTED, [[0], [1, 2, 3]])], alleles=[K.allele_rec([K.allele(203, del_len=2, ratio=0.75)])], align_id=[50, 51, 52, 53])
    bypassed = K.sample(reads, [K.obs(0, 205, del_len=1)], hap=[K.hap_rec(H.BYPASSED)], alleles=[K.allele_rec(status=H.BYPASSED)])
    samples = [bypassed, counted] if bypassed_sample == 0 else [counted, bypassed]
    want, _ = _table(samples, [(200, 210)])
    by = {k["pos"]: k for k in want}
    # the key the counted sample's region discovers exists for the bypassed sample's marks only if the counted sample came first
    assert by[203]["samples"][bypassed_sample]["is_haplotyping_bypassed"] == (0 if bypassed_sample == 0 else 1)
    assert by[205]["samples"][bypassed_sample]["is_haplotyping_bypassed"] == 1 and by[203]["active_region_id"] == 200


@pytest.mark.parametrize("status", [H.NO_READS, H.TOO_FEW_COVERING, H.DECLINED, "alleles_declined"])
def test_a_pending_pair(status):
    s0, regions = TM._pending_case(*((H.COUNTED, H.DECLINED) if status == "alleles_declined" else (status,)))
    want, totals = _table([s0], regions, pending_allowed=True)
    assert totals[3] == 1 and sum(bool(k["flags"] & T.AR_PENDING) for k in want) == 2


def _outside_allele_cap(d):
    d["alleles"]["recs"][0]["n_alleles"] += 1


def _outside_insert_cap(d):
    d["alleles"]["alleles"][0]["ins_off"] = len(d["alleles"]["insert_pool"]) - 1


def _outside_support_cap(d):
    d["haplotypes"]["recs"][0]["hap"][1]["count"] += 1


def _first_obs_off(d):
    d["intake"]["obs_off"][0] = 1


def _pool_case():
    """one region whose only record has an insert of two bytes and a support list that ends the pool"""
    return K.sample(["ACGT"] * 3, [K.obs(0, 190, del_len=1), K.obs(1, 191, del_len=1)], hap=[K.hap_rec(H.COUNTED, [[0], [1, 2]])],
                    alleles=[K.allele_rec([K.allele(200, ins="GA")])]), [(195, 205)]


def _host_call(samples, regions=(), caps=None, n_samples=None, mutate=None):
    """sk_indel_table's return value on model-form samples; mutate: applied to every sample's arrays before the call"""
    try:
        dev_samples = [K.device_sample(s) for s in samples]
        for d in dev_samples:
            if mutate:
                mutate(d)
        capi.indel_table(K.REF, K.REF_OFFSET, dev_samples, list(regions), raw=True, caps=caps)
    except capi.StrelkaAmdError as e:
        return str(e)
    return ""


def test_refusals_of_the_host_entry():
    capi.init(0)
    ok = K.deletions_case(2)
    assert _host_call([ok]) == ""
    assert "SK_MAX_SAMPLES" in _host_call([ok] * 9) and "SK_MAX_SAMPLES" in _host_call([])
    assert "iat above 2" in _host_call([K.deletions_case(2, iat=[0, 3])])
    assert "outside its read" in _host_call([K.sample(["ACGT"], [K.obs(0, 200, ins=(2, 3))])])
    bad = K.sample(["ACGT"] * 3, [], hap=[K.hap_rec(H.COUNTED, [[0], [1, 7]])], alleles=[K.allele_rec([K.allele(200, del_len=1)])])
    assert "support list names a read outside" in _host_call([bad], [(195, 205)])
    bad = K.sample(["ACGT"] * 3, [], hap=[K.hap_rec(H.COUNTED, [[0], [1, 2]])], alleles=[K.allele_rec([K.allele(200, del_len=1, hap_slot=2)])])
    assert "did not select" in _host_call([bad], [(195, 205)])
    # a record outside its pools, one pool at a time; offsets that do not begin at 0
    pool, pool_regions = _pool_case()
    assert _host_call([pool], pool_regions) == ""
    for mutate, which in ((_outside_allele_cap, "outside allele_cap"), (_outside_insert_cap, "outside insert_cap"), (_outside_support_cap, "outside support_cap"),
                          (_first_obs_off, "must begin at 0")):
        assert which in _host_call([pool], pool_regions, mutate=mutate), which
    # capacities one below the bounds: 2 observations, 0 records, 0 support, 8 read bases
    assert capi.indel_table_bounds(2, 0, 0, 8, 0) == (2, 2, 8)
    assert "key_cap" in _host_call([ok], caps=(1, 2, 8)) and "id_cap" in _host_call([ok], caps=(2, 1, 8)) and "insert_cap" in _host_call([ok], caps=(2, 2, 7))
    assert "negative size" in _host_call([ok], caps=(-1, 2, 8))
    assert capi.lib().sk_indel_table_key_bound(-1, 0) == -1 and capi.lib().sk_indel_table_scratch_bytes(9, 10, 10) == 0
    assert _host_call([ok]) == ""  # and the library goes on working


def _dev_table(samples, regions, n_regions=None, region_cap=None, expand_cap=None, key_cap=None, id_cap=None, insert_cap=None, prev_end_in=-1, mutate=None):
    """sk_indel_table_dev on uploaded arrays -> (dict of what it left, n_samples)"""
    import torch
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: None if t is None else t.data_ptr()
    m = len(regions)
    region_cap = m + 2 if region_cap is None else region_cap
    reg = np.zeros(max(region_cap, 1), capi.ACTIVE_REGION_DTYPE)
    for i, (b, e) in enumerate(regions):
        reg[i] = (b, e, 0)
    keep, structs, tot = [], [], dict(n_obs=0, n_alleles=0, n_support=0, n_bases=0, n_ins=0)
    for s in samples:
        ds = K.device_sample(s)
        if mutate:
            mutate(ds)
        st, arrays, sizes = capi.pack_indel_table_sample(ds, m)
        t = {}
        for name in ("read_off", "code", "obs_off", "obs", "align_id", "iat", "hap", "support", "recs", "alleles", "ins"):
            a = arrays[name]
            if a is None:
                t[name] = None
                continue
            pad = np.zeros(max(region_cap - m, 0) + 1, a.dtype) if name in ("hap", "recs") else np.zeros(1, a.dtype)
            t[name] = dev(np.concatenate([a, pad]).view(np.uint8))
        keep.append(t)
        structs.append(capi.IndelTableSample(st.n_reads, 0, p(t["read_off"]), p(t["code"]), p(t["obs_off"]), p(t["obs"]), st.obs_cap, p(t["align_id"]), p(t["iat"]), p(t["hap"]),
                                             p(t["support"]), st.support_cap, p(t["recs"]), p(t["alleles"]), st.allele_cap, p(t["ins"]), st.insert_cap))
        for k in tot:
            tot[k] += sizes[k]
    n_samples = len(samples)
    arr = (capi.IndelTableSample * n_samples)(*structs)
    bounds = capi.indel_table_bounds(tot["n_obs"], tot["n_alleles"], tot["n_support"], tot["n_bases"], tot["n_ins"])
    key_cap = bounds[0] if key_cap is None else key_cap
    id_cap = bounds[1] if id_cap is None else id_cap
    insert_cap = bounds[2] if insert_cap is None else insert_cap
    expand_cap = tot["n_obs"] + tot["n_alleles"] + tot["n_support"] if expand_cap is None else expand_cap
    d = dict(ref=dev(np.frombuffer(K.REF.encode(), np.uint8).copy()), regions=dev(reg.view(np.int32)), n=dev(np.array([m if n_regions is None else n_regions], np.int32)),
             keys=torch.full((max(key_cap, 1) * 56,), 0x5a, dtype=torch.uint8, device="cuda"), data=torch.full((max(key_cap, 1) * n_samples * 64,), 0x5a, dtype=torch.uint8, device="cuda"),
             ids=torch.zeros(max(id_cap, 1), dtype=torch.int32, device="cuda"), ins=torch.zeros(max(insert_cap, 1), dtype=torch.uint8, device="cuda"),
             totals=torch.full((4,), -1, dtype=torch.int64, device="cuda"), keep=keep)
    scratch_bytes = L.sk_indel_table_scratch_bytes(n_samples, expand_cap, region_cap)
    d["scratch"] = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    capi._check(L.sk_indel_table_dev(n_samples, C.addressof(arr), p(d["ref"]), K.REF_OFFSET, len(K.REF), p(d["regions"]), p(d["n"]), region_cap, prev_end_in, expand_cap,
                                     p(d["keys"]), key_cap, p(d["data"]), p(d["ids"]), id_cap, p(d["ins"]), insert_cap, p(d["totals"]), p(d["scratch"]), scratch_bytes,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return d, n_samples


def _dev_raw(d, n_samples):
    totals = d["totals"].cpu().numpy()
    nk = int(totals[0])
    return dict(keys=d["keys"].cpu().numpy()[:nk * 56].view(capi.INDEL_TABLE_KEY_DTYPE), data=d["data"].cpu().numpy()[:nk * n_samples * 64].view(capi.INDEL_TABLE_SAMPLE_DATA_DTYPE),
                id_pool=d["ids"].cpu().numpy().view(np.uint32)[:int(totals[1])], insert_pool=d["ins"].cpu().numpy()[:int(totals[2])], totals=totals)


def _two_sample_case():
    reads = ["ACGTACGT"] * 5
    s0 = K.sample(reads, [K.obs(0, 203, del_len=2), K.obs(1, 203, del_len=2, noise=1), K.obs(3, 220, ins=(1, 3))], align_id=[9, 8, 7, 6, 5], iat=[0, 1, 2, 0, 1],
                  hap=[K.hap_rec(H.COUNTED, [[0, 1], [2, 3, 4]]), K.hap_rec(H.BYPASSED)], alleles=[K.allele_rec([K.allele(203, del_len=2, ratio=0.6)]), K.allele_rec(status=H.BYPASSED)])
    s1 = K.sample(reads, [K.obs(2, 221, del_len=1)], hap=[K.hap_rec(H.COUNTED, [[0, 1, 2, 3, 4]]), K.hap_rec(H.COUNTED, [[0], [1, 2, 3]])],
                  alleles=[K.allele_rec(), K.allele_rec([K.allele(221, del_len=1, ratio=0.75), K.allele(222, K.MISMATCH, 1, "G", to_indel_buffer=0)])])
    return [s0, s1], [(200, 210), (218, 226)]


def test_device_entry_on_device_counts_below_the_caps():
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    samples, regions = _two_sample_case()
    want, totals = _table(samples, regions, prev_end_in=150)
    d, n_samples = _dev_table(samples, regions, region_cap=7, prev_end_in=150)
    capi._check(capi.lib().sk_check_device_errors())
    raw = _dev_raw(d, n_samples)
    _check_layout(raw, n_samples)
    assert capi.indel_table_records(raw["keys"], raw["data"], raw["id_pool"], raw["insert_pool"], n_samples) == want and raw["totals"].tolist() == totals
    assert d["keys"].cpu().numpy()[len(want) * 56:].tolist() == [0x5a] * (len(d["keys"]) - len(want) * 56)  # keys past totals[0] are not written
    # fewer regions on the device than the list holds: the second region's records and marks are not looked at
    d, _ = _dev_table(samples, regions, n_regions=1, region_cap=7, prev_end_in=150)
    capi._check(capi.lib().sk_check_device_errors())
    got = _dev_raw(d, n_samples)
    short = [dict(s, hap=s["hap"][:1], alleles=s["alleles"][:1]) for s in samples]
    want1, totals1 = T.indel_table(K.REF, K.REF_OFFSET, short, regions[:1], 150)
    assert capi.indel_table_records(got["keys"], got["data"], got["id_pool"], got["insert_pool"], n_samples) == want1 and got["totals"].tolist() == totals1


def test_device_entry_raises_the_flag_and_leaves_an_empty_table():
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    samples, regions = _two_sample_case()
    want, totals = T.indel_table(K.REF, K.REF_OFFSET, samples, regions, -1)
    n_exp = 4 + 2 + 6  # observations, records handed to the buffer, their supporting reads
    for kw in (dict(expand_cap=n_exp - 1), dict(key_cap=totals[0] - 1), dict(id_cap=totals[1] - 1), dict(insert_cap=totals[2] - 1)):
        d, n_samples = _dev_table(samples, regions, **kw)
        assert L.sk_check_device_errors() != 0 and "sk_indel_table_dev" in capi.last_error() and L.sk_check_device_errors() == 0, kw
        assert d["totals"].cpu().numpy().tolist() == [0, 0, 0, 0], kw
    d, n_samples = _dev_table(samples, regions, expand_cap=n_exp, key_cap=totals[0], id_cap=totals[1], insert_cap=totals[2])  # exactly what the arrays hold: enough
    capi._check(L.sk_check_device_errors())
    assert d["totals"].cpu().numpy().tolist() == totals
    for bad in (K.deletions_case(2, iat=[0, 3]), K.sample(["ACGT"], [K.obs(0, 200, ins=(2, 3))]),
                K.sample(["ACGT"] * 3, [], hap=[K.hap_rec(H.COUNTED, [[0], [1, 7]])] * 2, alleles=[K.allele_rec([K.allele(200, del_len=1)]), K.allele_rec()])):
        d, n_samples = _dev_table([bad], regions if bad["hap"] else [])
        assert L.sk_check_device_errors() != 0 and "sk_indel_table_dev" in capi.last_error()
        assert d["totals"].cpu().numpy().tolist() == [0, 0, 0, 0]
    pool, pool_regions = _pool_case()
    for mutate in (_outside_allele_cap, _outside_insert_cap, _outside_support_cap, _first_obs_off):  # a record outside its pools; offsets that do not begin at 0
        d, n_samples = _dev_table([pool], pool_regions, mutate=mutate)
        assert L.sk_check_device_errors() != 0 and "sk_indel_table_dev" in capi.last_error(), mutate.__name__
        assert d["totals"].cpu().numpy().tolist() == [0, 0, 0, 0], mutate.__name__
    d, n_samples = _dev_table([pool], pool_regions)
    capi._check(L.sk_check_device_errors())
    assert d["totals"].cpu().numpy().tolist() == T.indel_table(K.REF, K.REF_OFFSET, [pool], pool_regions)[1]
    assert _table(samples, regions)[1] == totals  # and the library goes on working


def test_indel_table_behind_the_device_chain_on_one_stream():
    """per sample sk_read_intake_dev -> sk_region_haplotypes_dev -> sk_region_alleles_dev, then sk_indel_table_dev, all on one stream with no
    host copy in between, on the recorded two-sample scene: against the model, hence against the reference's map"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    from tests import test_region_haplotypes as RH
    capi.init(0)
    L = capi.lib()
    sc = next(s for s in T.golden() if s["name"] == "two_samples_one_deletion")
    samples, regions = T.scene_samples(sc)
    want, totals = T.indel_table(sc["ref"], sc["ref_offset"], samples, regions, sc["prev_end_in"])
    assert T.as_recorded(want) == sc["keys"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    region_cap, max_hap_len = len(regions) + 3, 256
    reg = np.zeros(region_cap, capi.ACTIVE_REGION_DTYPE)
    for i, (b, e) in enumerate(regions):
        reg[i] = (b, e, 0)
    d_regions, d_n = dev(reg.view(np.int32)), dev(np.array([len(regions)], np.int32))
    opt = capi.intake_options()
    opt.max_indel_size = sc["max_indel_size"]
    allele_cap, insert_cap = capi.region_alleles_bounds(region_cap, max_hap_len)
    a_scratch_bytes = L.sk_region_alleles_scratch_bytes(region_cap, max_hap_len)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep, structs, n_obs_cap, n_bases = [], [], 0, 0
    for sm in samples:
        c = dict(ref=sc["ref"], ref_offset=sc["ref_offset"], reads=sm["reads"], low=sm["low"], fwd=sm["fwd"], max_indel_size=sc["max_indel_size"], buf_begin=sm["buf_begin"],
                 buf_end=sm["buf_end"], ploidy=sm["ploidy"])
        n = len(sm["reads"])
        d = RH._dev_upload(c, region_cap)
        t, n_segs = d["t"], d["n_segs"]
        cap = capi.read_intake_obs_bound(n_segs)
        x = dict(reads=torch.zeros(n * 16, dtype=torch.uint8, device="cuda"), obs_off=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                 obs=torch.zeros(cap * 32, dtype=torch.uint8, device="cuda"), sites=torch.zeros(1, dtype=torch.int64, device="cuda"), cand=torch.zeros(1, dtype=torch.uint8, device="cuda"),
                 arecs=torch.zeros(region_cap * 72, dtype=torch.uint8, device="cuda"), alleles=torch.zeros(allele_cap * 56, dtype=torch.uint8, device="cuda"),
                 ins=torch.zeros(insert_cap, dtype=torch.uint8, device="cuda"), atotals=torch.zeros(2, dtype=torch.int64, device="cuda"), prev=torch.zeros(1, dtype=torch.int32, device="cuda"),
                 ascratch=torch.zeros(a_scratch_bytes, dtype=torch.uint8, device="cuda"), align_id=dev(np.array(sm["align_id"] + [0], np.uint32).view(np.int32)),
                 iat=dev(np.array(sm["iat"] + [0], np.uint8)))
        i_scratch_bytes = L.sk_read_intake_scratch_bytes(n, n_segs, 0)
        x["iscratch"] = torch.zeros(max(i_scratch_bytes, 1), dtype=torch.uint8, device="cuda")
        capi._check(L.sk_read_intake_dev(p(d["ref"]), sc["ref_offset"], len(sc["ref"]), n, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]), C.byref(opt), 0, 0,
                                         p(x["reads"]), p(x["obs_off"]), p(x["obs"]), cap, p(x["sites"]), p(x["cand"]), p(x["iscratch"]), i_scratch_bytes, st))
        d["obs_off"], d["obs"] = x["obs_off"], x["obs"]
        RH._dev_launch(c, d, d_regions, d_n, st)
        capi._check(L.sk_region_alleles_dev(p(d["ref"]), sc["ref_offset"], len(sc["ref"]), p(d_regions), p(d_n), region_cap, p(d["recs"]), p(d["seq"]), d["seq_cap"],
                                            sc["max_indel_size"], max_hap_len, sc["prev_end_in"], p(x["arecs"]), p(x["alleles"]), allele_cap, p(x["ins"]), insert_cap,
                                            p(x["atotals"]), p(x["prev"]), p(x["ascratch"]), a_scratch_bytes, st))
        keep.append((d, x))
        q = lambda tensor: tensor.data_ptr()
        structs.append(capi.IndelTableSample(n, 0, q(t[0]), q(t[1]), q(x["obs_off"]), q(x["obs"]), cap, q(x["align_id"]), q(x["iat"]), q(d["recs"]), q(d["support"]),
                                             d["support_cap"], q(x["arecs"]), q(x["alleles"]), allele_cap, q(x["ins"]), insert_cap))
        n_obs_cap += cap
        n_bases += sum(len(r["code"]) for r in sm["reads"])
    n_samples = len(samples)
    arr = (capi.IndelTableSample * n_samples)(*structs)
    expand_cap = 4096  # (the counts are on the device: the caller's estimate)
    key_cap, id_cap, ins_cap = 512, 4096, n_bases + 1024
    out = dict(keys=torch.zeros(key_cap * 56, dtype=torch.uint8, device="cuda"), data=torch.zeros(key_cap * n_samples * 64, dtype=torch.uint8, device="cuda"),
               ids=torch.zeros(id_cap, dtype=torch.int32, device="cuda"), ins=torch.zeros(ins_cap, dtype=torch.uint8, device="cuda"),
               totals=torch.full((4,), -1, dtype=torch.int64, device="cuda"))
    scratch_bytes = L.sk_indel_table_scratch_bytes(n_samples, expand_cap, region_cap)
    scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    capi._check(L.sk_indel_table_dev(n_samples, C.addressof(arr), keep[0][0]["ref"].data_ptr(), sc["ref_offset"], len(sc["ref"]), d_regions.data_ptr(), d_n.data_ptr(), region_cap,
                                     sc["prev_end_in"], expand_cap, out["keys"].data_ptr(), key_cap, out["data"].data_ptr(), out["ids"].data_ptr(), id_cap, out["ins"].data_ptr(),
                                     ins_cap, out["totals"].data_ptr(), scratch.data_ptr(), scratch_bytes, st))
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    raw = _dev_raw(out, n_samples)
    _check_layout(raw, n_samples)
    assert capi.indel_table_records(raw["keys"], raw["data"], raw["id_pool"], raw["insert_pool"], n_samples) == want and raw["totals"].tolist() == totals
