"""Region alleles on the device (sk_region_alleles, csrc/region_alleles.hip): every field of every record equals the loop model
(tests/alleles_model.py, itself pinned to vectors recorded from the reference by tests/test_region_alleles_model.py).

All four decline reasons are reached here.  A haplotype above max_hap_len and a left shift that would not end come from input.  The
aligner's beginPos > 0 cannot happen with the detector's scores (a leading reference base is a required edge deletion), and a key
whose haplotype ids add up to more than 3 needs one key twice in one haplotype, which no path of the aligner's holds; both are
reached through the test hook sk_debug_region_alleles (the first by dropping the required edge deletion from the scores, the second
by counting a repeated key's id twice), and the second rule is driven in the model with a replaced aligner
(tests/test_region_alleles_model.py)."""
import ctypes as C

import numpy as np
import pytest

from strelka_amd import capi
from tests import alleles_model as A
from tests import haplotype_model as H
from tests import region_haplotype_cases as R
from tests import test_region_haplotypes as T

pytestmark = pytest.mark.gpu

MS, IN, DE = R.MS, R.IN, R.DE


def _check_layout(raw):
    """the records and the insert bytes lie back to back in region order, every record's bytes inside its region's, totals count them"""
    at = at_ins = 0
    for r in raw["recs"]:
        assert (int(r["allele_off"]), int(r["insert_off"])) == (at, at_ins) and int(r["pad"]) == 0
        ins = at_ins
        for a in raw["alleles"][at:at + int(r["n_alleles"])]:
            assert int(a["ins_off"]) == ins and int(a["pad"]) == 0
            ins += int(a["ins_len"])
        at += int(r["n_alleles"])
        at_ins += int(r["n_insert_bytes"])
        assert ins == at_ins
        if int(r["n_alleles"]) == 0:
            assert r["score"].tolist()[int(r["n_alt"]):] == [0] * (2 - int(r["n_alt"]))
    assert raw["totals"].tolist() == [at, at_ins] and len(raw["alleles"]) == at and len(raw["insert_pool"]) == at_ins


def _alleles(c, hap_raw, hap_model, prev_end_in=-1, max_hap_len=1024, what="", declines=()):
    """device against model for regions whose haplotype records are given both ways -> the model's records"""
    got = capi.region_alleles(c["ref"], c["ref_offset"], c["regions"], hap_raw, c["max_indel_size"], max_hap_len, prev_end_in, raw=True)
    want, prev_end_out = A.region_alleles(c["ref"], c["ref_offset"], c["regions"], hap_model, c["max_indel_size"], max_hap_len, prev_end_in)
    recs = capi.region_allele_records(got["recs"], got["alleles"], got["insert_pool"])
    assert len(recs) == len(want) and got["prev_end_out"] == prev_end_out
    for i, (g, w) in enumerate(zip(recs, want)):
        assert g == w, "%s region %d %s" % (what, i, c["regions"][i])
        if i not in declines:  # no region may decline unless the test was built for it
            assert not (w["status"] == H.DECLINED and w["reason"] >= A.DECLINE_BEGIN_POS), "%s region %d declined" % (what, i)
    _check_layout(got)
    return want


def _run(c, what="", **kw):
    """the chain of host entries on a case of reads"""
    capi.init(0)
    opt = capi.intake_options()
    opt.max_indel_size = c["max_indel_size"]
    hap_raw = capi.region_haplotypes(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], c["regions"], c["buf_begin"], c["buf_end"], c["ploidy"], opt=opt, raw=True)
    return _alleles(c, hap_raw, R.model(c), what=what, **kw)


def _crafted(regions, ref=R.REF, ref_offset=R.REF_OFFSET, max_indel_size=49):
    """regions: [(begin, end, status, reason, n_reads_aligned, [(haplotype, count)])] -> (case, the haplotype records as
    sk_region_haplotypes leaves them, the same as the model's)"""
    recs = np.zeros(len(regions), capi.REGION_HAPLOTYPES_DTYPE)
    seq, model, n_support = [], [], 0
    for i, (begin, end, status, reason, n_aligned, haps) in enumerate(regions):
        seg = "".join(A.M.ref_char(ref, ref_offset, p) for p in range(begin, end))
        recs[i]["status"], recs[i]["reason"], recs[i]["n_reads_aligned"], recs[i]["n_reads_covering"], recs[i]["n_selected"] = status, reason, n_aligned, n_aligned, len(haps)
        m = dict(status=status, reason=reason, n_reads_aligned=n_aligned, n_reads_covering=n_aligned, haps=[])
        for k, (s, count) in enumerate(haps):
            recs[i]["hap"][k] = (sum(len(x) for x in seq), n_support, len(s), count, int(s == seg), 0)
            m["haps"].append(dict(seq=s, count=count, is_reference=int(s == seg), support=list(range(n_support, n_support + count))))
            seq.append(s)
            n_support += count
        model.append(m)
    c = dict(ref=ref, ref_offset=ref_offset, regions=[(r[0], r[1]) for r in regions], max_indel_size=max_indel_size)
    raw = dict(recs=recs, seq_pool=np.frombuffer("".join(seq).encode("latin-1"), np.uint8).copy() if seq else np.zeros(0, np.uint8))
    return c, raw, model


def _sub_any(s, at):
    return s[:at] + R.other(s[at]) + s[at + 1:]


def _seg(b, e):
    return R.REF[b - R.REF_OFFSET:e - R.REF_OFFSET]


def _sub(s, at):
    return s[:at] + R.other(s[at]) + s[at + 1:]


def test_region_lengths_1_2_63_64_65_and_250():
    c = R.case(T._long_reads(), [(200, 201), (200, 202), (200, 263), (200, 264), (200, 265), (150, 400), (263, 265), (219, 220)])
    want = _run(c, "lengths")
    assert [r["status"] for r in want] == [H.COUNTED] * 8 and [r["n_alt"] for r in want[:6]] == [1] * 6 and want[6]["n_alt"] == 2
    assert len(want[0]["alleles"]) >= 1  # (the regions after it begin below their prev_end: most of their keys belong to the region before)
    c["ploidy"] = 1
    _run(c, "lengths, haploid")
    n_keys = 0
    for region in c["regions"][:6]:  # each as a list of its own: nothing lies below prev_end
        n_keys += len(_run(R.case(T._long_reads(), [region]), "region %s alone" % (region,))[0]["alleles"])
    assert n_keys >= 6


@pytest.mark.parametrize("hap_len", [1, 63, 64, 65, 128, 129])
def test_haplotype_lengths_around_the_aligners_strips(hap_len):
    capi.init(0)
    # the region's segment with a substitution, then a deletion or an insertion that brings it to hap_len
    span = {1: 2, 63: 64, 64: 64, 65: 64, 128: 120, 129: 130}[hap_len]
    seg = _seg(200, 200 + span)
    first = _sub(seg, span // 2)[:hap_len] if hap_len <= span else _sub(seg, 3)[:span - 2] + "GATTACAT"[:hap_len - span] + seg[span - 2:]
    second = seg[:span // 3] + "T" * max(hap_len - span, 0) + seg[span // 3 + max(span - hap_len, 0):] if hap_len != span else _sub(seg, span // 3)
    assert len(first) == len(second) == hap_len and seg not in (first, second)
    c, raw, model = _crafted([(200, 200 + span, H.COUNTED, 0, 9, [(seg, 4), (first, 3), (second, 2)]), (200, 200 + span, H.COUNTED, 0, 5, [(second, 5)])])
    want = _alleles(c, raw, model, what="haplotype of %d" % hap_len)
    assert want[0]["n_alt"] == 2 and want[0]["hap_slot"] == [1, 2] and want[1]["n_alt"] == 1 and want[1]["hap_slot"] == [0]
    assert len(want[0]["alleles"]) + len(want[1]["alleles"]) >= 2
    _alleles(c, raw, model, max_hap_len=max(hap_len, 1), what="max_hap_len at the length")


def _dev_alleles(c, raw, n_regions, region_cap, max_hap_len=1024, prev_end_in=-1, allele_cap=None, insert_cap=None):
    """sk_region_alleles_dev on uploaded host arrays -> dict of what it left"""
    import torch
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    regions = np.zeros(max(region_cap, 1), capi.ACTIVE_REGION_DTYPE)
    for i, (b, e) in enumerate(c["regions"]):
        regions[i] = (b, e, 0)
    hap = np.zeros(max(region_cap, 1), capi.REGION_HAPLOTYPES_DTYPE)
    hap[:len(raw["recs"])] = raw["recs"]
    seq = np.concatenate([raw["seq_pool"], np.zeros(8, np.uint8)])
    bound = capi.region_alleles_bounds(region_cap, max_hap_len)
    allele_cap = bound[0] if allele_cap is None else allele_cap
    insert_cap = bound[1] if insert_cap is None else insert_cap
    d = dict(ref=dev(np.frombuffer(c["ref"].encode(), np.uint8).copy()), regions=dev(regions.view(np.int32)), n=dev(np.array([n_regions], np.int32)),
             hap=dev(hap.view(np.uint8)), seq=dev(seq), recs=torch.full((max(region_cap, 1) * 72,), 0x5a, dtype=torch.uint8, device="cuda"),
             alleles=torch.zeros(max(allele_cap, 1) * 56, dtype=torch.uint8, device="cuda"), ins=torch.zeros(max(insert_cap, 1), dtype=torch.uint8, device="cuda"),
             totals=torch.full((2,), -1, dtype=torch.int64, device="cuda"), prev=torch.full((1,), -7, dtype=torch.int32, device="cuda"))
    scratch_bytes = L.sk_region_alleles_scratch_bytes(region_cap, max_hap_len)
    d["scratch"] = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    capi._check(L.sk_region_alleles_dev(p(d["ref"]), c["ref_offset"], len(c["ref"]), p(d["regions"]), p(d["n"]), region_cap, p(d["hap"]), p(d["seq"]), len(raw["seq_pool"]),
                                        c["max_indel_size"], max_hap_len, prev_end_in, p(d["recs"]), p(d["alleles"]), allele_cap, p(d["ins"]), insert_cap, p(d["totals"]),
                                        p(d["prev"]), p(d["scratch"]), scratch_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return d


def _dev_raw(d, n_regions):
    totals = d["totals"].cpu().numpy()
    return dict(recs=d["recs"].cpu().numpy()[:n_regions * 72].view(capi.REGION_ALLELES_DTYPE), alleles=d["alleles"].cpu().numpy().view(capi.REGION_ALLELE_DTYPE)[:int(totals[0])],
                insert_pool=d["ins"].cpu().numpy()[:int(totals[1])], totals=totals, prev_end_out=int(d["prev"].cpu()[0]))


@pytest.mark.parametrize("n_regions", [0, 1, 2, 65])
def test_region_counts_below_region_cap(n_regions):
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    spec = []
    for i in range(n_regions):
        b = 150 + 3 * i
        span = 1 + i % 7
        seg = _seg(b, b + span)
        alts = [(_sub(seg, i % span), 3)] + ([(seg[:span // 2] + "GA" + seg[span // 2:], 3)] if i % 3 == 0 else [])
        spec.append((b, b + span, H.COUNTED, 0, 10, [(seg, 4)] * (i % 2) + alts))
    c, raw, model = _crafted(spec)
    want = _alleles(c, raw, model, prev_end_in=33, what="%d regions" % n_regions)
    cap = n_regions + 3
    d = _dev_alleles(c, raw, n_regions, cap, prev_end_in=33)
    capi._check(capi.lib().sk_check_device_errors())
    got = _dev_raw(d, n_regions)
    _check_layout(got)
    assert capi.region_allele_records(got["recs"], got["alleles"], got["insert_pool"]) == want
    assert got["prev_end_out"] == (spec[-1][1] if spec else 33)
    assert d["recs"].cpu().numpy()[n_regions * 72:].tolist() == [0x5a] * (3 * 72)  # slots past n_regions are not looked at


@pytest.mark.parametrize("name", [s["name"] for s in A.golden()])
def test_recorded_vectors(name):
    """every recorded region with the prev_end it was recorded at: the records against the model, and replayed against what the
    reference's IndelBuffer and CandidateSnvBuffer held"""
    capi.init(0)
    sc = next(s for s in A.golden() if s["name"] == name)
    for g in sc["regions"]:
        c = R.case(sc["reads"], [(g["begin"], g["end"])], low=sc["low"], fwd=sc["fwd"], buf=(sc["buf_begin"], sc["buf_end"]), ploidy=g["ploidy"], ref=sc["ref"],
                   ref_offset=sc["ref_offset"], max_indel_size=sc["max_indel_size"])
        what = "%s [%d, %d) ploidy %d prev_end %d" % (name, g["begin"], g["end"], g["ploidy"], g["prev_end"])
        opt = capi.intake_options()
        opt.max_indel_size = c["max_indel_size"]
        hap_raw = capi.region_haplotypes(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], c["regions"], c["buf_begin"], c["buf_end"], c["ploidy"], opt=opt, raw=True)
        hap_model = R.model(c)
        want = _alleles(c, hap_raw, hap_model, prev_end_in=g["prev_end"], what=what)
        got, _ = capi.region_alleles(c["ref"], c["ref_offset"], c["regions"], hap_raw, c["max_indel_size"], 1024, g["prev_end"])
        assert A.replay(g["begin"], got[0], hap_model[0]) == (g["keys"], g["snvs"]), what
        assert want[0]["status"] == H.COUNTED


def test_statuses_pass_through_and_prev_end_advances():
    capi.init(0)
    seg = lambda b, e: _seg(b, e)
    # the SNV at 209 lies in [204, 210) and in [209, 215): the second region leaves it to the first whatever lies between them
    alt_a = _sub(seg(204, 210), 5)
    alt_b = _sub(seg(209, 215), 0)
    spec = [(190, 200, H.BYPASSED, 0, 0, []), (204, 210, H.COUNTED, 0, 8, [(seg(204, 210), 5), (alt_a, 3)]), (209, 215, H.COUNTED, 0, 8, [(alt_b, 8)]),
            (212, 216, H.NO_READS, 0, 0, []), (213, 220, H.COUNTED, 0, 6, [(_sub(seg(213, 220), 1), 6)]), (218, 230, H.TOO_FEW_COVERING, 0, 9, []),
            (225, 231, H.DECLINED, H.DECLINE_GROUPS, 60, []), (229, 236, H.COUNTED, 0, 6, [(_sub(seg(229, 236), 0), 3), (_sub(seg(229, 236), 2), 3)]),
            (240, 250, H.COUNTED, 0, 2, []), (245, 255, H.COUNTED, 0, 7, [(seg(245, 255), 7)])]
    c, raw, model = _crafted(spec)
    want = _alleles(c, raw, model, prev_end_in=195, what="statuses")
    assert [r["status"] for r in want] == [s[2] for s in spec] and want[6]["reason"] == H.DECLINE_GROUPS
    assert [r["prev_end"] for r in want] == [195] + [s[1] for s in spec[:-1]]
    assert want[1]["alleles"][0]["pos"] == 209 and want[2]["alleles"] == []       # the shared base
    assert want[4]["alleles"] == [] and want[4]["n_alt"] == 1                      # 214 < prev_end 216, though the region between had no reads
    assert [a["pos"] for a in want[7]["alleles"]] == [231]                         # 229 < prev_end 231
    assert want[8]["n_alt"] == 0 and want[9]["n_alt"] == 0 and want[9]["do_not_add_mismatches"] == 1


def test_declines():
    capi.init(0)
    # a haplotype of 9 with max_hap_len 8; the region after it is answered
    seg = _seg(200, 208)
    c, raw, model = _crafted([(200, 208, H.COUNTED, 0, 6, [(seg[:4] + "A" + seg[4:], 6)]), (210, 214, H.COUNTED, 0, 6, [(_sub(_seg(210, 214), 1), 6)])])
    want = _alleles(c, raw, model, max_hap_len=8, what="hap_len", declines=(0,))
    assert (want[0]["status"], want[0]["reason"], want[0]["alleles"]) == (H.DECLINED, A.DECLINE_HAP_LEN, []) and len(want[1]["alleles"]) == 1
    assert _alleles(c, raw, model, max_hap_len=9, what="hap_len 9")[0]["status"] == H.COUNTED
    # an insertion of N at the start of a reference that begins with N: the reference's left-shift loop would not end
    ref = "N" * 10 + R.REF[10:]
    c, raw, model = _crafted([(100, 104, H.COUNTED, 0, 6, [("NNNNNN", 6)]), (110, 114, H.COUNTED, 0, 6, [(_sub(ref[10:14], 1), 6)])], ref=ref)
    want = _alleles(c, raw, model, what="left shift", declines=(0,))
    assert (want[0]["status"], want[0]["reason"]) == (H.DECLINED, A.DECLINE_LEFT_SHIFT) and len(want[1]["alleles"]) == 1
    # beginPos > 0: only without the required edge deletion (see the module's text)
    seg = _seg(200, 212)
    c, raw, model = _crafted([(200, 212, H.COUNTED, 0, 6, [(seg[6:], 6)])])
    L = capi.lib()
    try:
        L.sk_debug_region_alleles(1, 0)
        got, _ = capi.region_alleles(c["ref"], c["ref_offset"], c["regions"], raw)
    finally:
        L.sk_debug_region_alleles(0, 0)
    assert (got[0]["status"], got[0]["reason"], got[0]["alleles"], got[0]["n_alt"]) == (H.DECLINED, A.DECLINE_BEGIN_POS, [], 0)
    want = _alleles(c, raw, model, what="edge deletion")
    assert [(a["type"], a["del_len"]) for a in want[0]["alleles"]] == [(A.INDEL, 6)]
    # an id sum above 3: the same deletion in both alternates with the repeat's id counted twice, 1 + 2 * 2; the region after it is answered,
    # and so is a region whose alternates share nothing
    seg = _seg(200, 212)
    both = seg[:4] + seg[7:]
    spec = [(200, 212, H.COUNTED, 0, 7, [(both, 4), (_sub(both, 7), 3)]), (214, 220, H.COUNTED, 0, 6, [(_sub(_seg(214, 220), 1), 3), (_sub(_seg(214, 220), 3), 3)])]
    c, raw, model = _crafted(spec)
    want = _alleles(c, raw, model, what="shared deletion")
    assert want[0]["alleles"][0]["id_sum"] == 3 and want[0]["alleles"][1]["same_as"] == 0
    try:
        L.sk_debug_region_alleles(0, 1)
        got, _ = capi.region_alleles(c["ref"], c["ref_offset"], c["regions"], raw)
    finally:
        L.sk_debug_region_alleles(0, 0)
    assert (got[0]["status"], got[0]["reason"], got[0]["alleles"], got[0]["n_alt"], got[0]["prev_end"]) == (H.DECLINED, A.DECLINE_ID_SUM, [], 0, -1)
    assert got[1] == want[1] and len(got[1]["alleles"]) == 2
    assert _alleles(c, raw, model, what="after the hook") == want


@pytest.mark.parametrize("n_regions", [1025, 2100])
def test_more_regions_than_one_scan_chunk_and_than_the_grid(n_regions):
    """above 1 024 regions the two scans carry from chunk to chunk; above 2 048 a workgroup of A2 and A4 takes a second slot, with the LDS
    table of the slot before"""
    capi.init(0)
    ref = "".join(np.random.default_rng(5).choice(list("ACGT"), 4 * n_regions + 64))
    spec = []
    for i in range(n_regions):
        b = 100 + 4 * i
        span = 3 + i % 4
        seg = ref[b - 100:b - 100 + span]
        kind = i % 5
        if kind == 0:
            spec.append((b, b + span, H.NO_READS, 0, 0, []))
        elif kind == 1:
            spec.append((b, b + span, H.COUNTED, 0, 5, [(seg, 5)]))
        else:
            alts = [(_sub_any(seg, i % span), 3)] + ([(seg[:1] + "GA" + seg[1:], 2)] if kind == 3 else []) + ([(seg[:1] + seg[2:], 2)] if kind == 4 else [])
            spec.append((b, b + span, H.COUNTED, 0, 9, [(seg, 4)] + alts))
    c, raw, model = _crafted(spec, ref=ref)
    want = _alleles(c, raw, model, max_hap_len=16, prev_end_in=50, what="%d regions" % n_regions)
    assert sum(len(r["alleles"]) for r in want) >= n_regions // 2 and want[-1]["prev_end"] == spec[-2][1]
    assert sum(1 for r in want[2048:] if r["alleles"]) >= (20 if n_regions > 2048 else 0)


def test_refused_inputs_and_capacities():
    capi.init(0)
    L = capi.lib()
    seg = _seg(200, 208)
    ok = [(200, 208, H.COUNTED, 0, 6, [(_sub(seg, 2), 6)])]
    c, raw, model = _crafted(ok)

    def call(c, raw, max_hap_len=1024, allele_cap=None, insert_cap=None, seq_len=None):
        reg = np.zeros(len(c["regions"]), capi.ACTIVE_REGION_DTYPE)
        for i, (b, e) in enumerate(c["regions"]):
            reg[i] = (b, e, 0)
        bound = capi.region_alleles_bounds(len(reg), 1024 if not 1 <= max_hap_len <= 1024 else max_hap_len)
        allele_cap = bound[0] if allele_cap is None else allele_cap
        insert_cap = bound[1] if insert_cap is None else insert_cap
        out = [np.zeros(len(reg), capi.REGION_ALLELES_DTYPE), np.zeros(max(allele_cap, 1), capi.REGION_ALLELE_DTYPE), np.zeros(max(insert_cap, 1), np.uint8), np.zeros(2, np.int64),
               np.zeros(1, np.int32)]
        ref = c["ref"].encode()
        return L.sk_region_alleles(ref, c["ref_offset"], len(ref), capi._p(reg), len(reg), capi._p(raw["recs"]), capi._p(raw["seq_pool"]),
                                   len(raw["seq_pool"]) if seq_len is None else seq_len, 49, max_hap_len, -1, capi._p(out[0]), capi._p(out[1]), allele_cap, capi._p(out[2]),
                                   insert_cap, capi._p(out[3]), capi._p(out[4]))
    assert call(c, raw) == 0
    for kw, which in ((dict(max_hap_len=0), "max_hap_len"), (dict(max_hap_len=1025), "max_hap_len"), (dict(allele_cap=2 * 1274 - 1), "allele_cap"),
                      (dict(insert_cap=2047), "insert_cap"), (dict(allele_cap=-1), "negative size"), (dict(seq_len=7), "outside seq_pool")):
        assert call(c, raw, **kw) != 0 and which in capi.last_error(), kw
    c2, raw2, _ = _crafted([(200, 451, H.COUNTED, 0, 6, [("ACGT", 6)])])
    assert call(c2, raw2) != 0 and "SK_HAP_MAX_REF_SPAN" in capi.last_error()
    c2, raw2, _ = _crafted([(200, 208, H.COUNTED, 0, 9, [(_sub(seg, 1), 3), (_sub(seg, 2), 3), (_sub(seg, 3), 3)])])
    assert call(c2, raw2) != 0 and "more than two alternate" in capi.last_error()
    if L.sk_broker_client():
        return
    # the device entry: the same input raises the sticky flag and the region is bypassed; so does room below the bound of the regions there are
    d = _dev_alleles(c2, raw2, 1, 4)
    assert L.sk_check_device_errors() != 0 and "sk_region_alleles_dev" in capi.last_error() and L.sk_check_device_errors() == 0
    got = _dev_raw(d, 1)
    assert (int(got["recs"][0]["status"]), got["totals"].tolist()) == (H.BYPASSED, [0, 0])
    d = _dev_alleles(c, raw, 1, 1, allele_cap=2 * 1274 - 1)
    assert L.sk_check_device_errors() != 0 and "sk_region_alleles_dev" in capi.last_error()
    got = _dev_raw(d, 1)
    assert (int(got["recs"][0]["status"]), got["totals"].tolist()) == (H.BYPASSED, [0, 0])
    want = _alleles(c, raw, model, what="after the refusals")  # and the library goes on working
    assert len(want[0]["alleles"]) == 1


def test_five_calls_on_one_stream_on_the_seeded_window():
    """sk_read_intake_dev -> sk_ref_anchors_dev -> sk_active_regions_dev -> sk_region_haplotypes_dev -> sk_region_alleles_dev on one stream,
    no host copy in between, against the host-array entries chained by the caller"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    c, intake, anchor, regions, hap_want = R.seeded_window_model()
    capi.init(0)
    L = capi.lib()
    max_hap_len = 256
    want = _run(c, "host chain", max_hap_len=max_hap_len)
    assert sum(1 for r in want if r["n_alt"] >= 1) * 2 >= len(want) and sum(1 for r in want for a in r["alleles"] if a["type"] == A.INDEL) >= 5
    n = len(c["reads"])
    win_begin, n_pos = c["win_begin"], c["n_pos"]
    region_cap = capi.active_regions_bound(n_pos)
    d = T._dev_upload(c, region_cap)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    d_ref, t, n_segs = d["ref"], d["t"], d["n_segs"]
    cap = capi.read_intake_obs_bound(n_segs)
    d_reads = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_obs_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_obs = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    d_sites = torch.zeros(n_pos, dtype=torch.int64, device="cuda")
    d_cand = torch.zeros(n_pos, dtype=torch.uint8, device="cuda")
    scratch_bytes = L.sk_read_intake_scratch_bytes(n, n_segs, n_pos)
    d_scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    d_anchor = torch.zeros(n_pos, dtype=torch.uint8, device="cuda")
    d_state_in = dev(capi.ar_state_initial().view(np.int32))
    d_state_out = torch.zeros(6, dtype=torch.int32, device="cuda")
    d_regions = torch.zeros(region_cap * 3, dtype=torch.int32, device="cuda")
    d_n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    allele_cap, insert_cap = capi.region_alleles_bounds(region_cap, max_hap_len)
    a = dict(recs=torch.full((region_cap * 72,), 0x5a, dtype=torch.uint8, device="cuda"), alleles=torch.zeros(allele_cap * 56, dtype=torch.uint8, device="cuda"),
             ins=torch.zeros(insert_cap, dtype=torch.uint8, device="cuda"), totals=torch.full((2,), -1, dtype=torch.int64, device="cuda"),
             prev=torch.full((1,), -7, dtype=torch.int32, device="cuda"))
    a_scratch_bytes = L.sk_region_alleles_scratch_bytes(region_cap, max_hap_len)
    a_scratch = torch.zeros(a_scratch_bytes, dtype=torch.uint8, device="cuda")
    opt = capi.intake_options()
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi._check(L.sk_read_intake_dev(p(d_ref), c["ref_offset"], len(c["ref"]), n, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]), C.byref(opt),
                                     win_begin, n_pos, p(d_reads), p(d_obs_off), p(d_obs), cap, p(d_sites), p(d_cand), p(d_scratch), scratch_bytes, st))
    capi._check(L.sk_ref_anchors_dev(p(d_ref), c["ref_offset"], len(c["ref"]), win_begin + 1, None, win_begin, n_pos, p(d_anchor), 0, None, None, st))
    capi._check(L.sk_active_regions_dev(win_begin, n_pos, p(d_sites), p(d_cand), p(d_anchor), p(d_state_in), p(d_state_out), p(d_regions), region_cap, p(d_n), st))
    d["obs_off"], d["obs"] = d_obs_off, d_obs
    T._dev_launch(c, d, d_regions, d_n, st)
    capi._check(L.sk_region_alleles_dev(p(d_ref), c["ref_offset"], len(c["ref"]), p(d_regions), p(d_n), region_cap, p(d["recs"]), p(d["seq"]), d["seq_cap"],
                                        c["max_indel_size"], max_hap_len, -1, p(a["recs"]), p(a["alleles"]), allele_cap, p(a["ins"]), insert_cap, p(a["totals"]),
                                        p(a["prev"]), p(a_scratch), a_scratch_bytes, st))
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    assert int(d_n.cpu()[0]) == len(regions)
    got = _dev_raw(a, len(regions))
    _check_layout(got)
    recs = capi.region_allele_records(got["recs"], got["alleles"], got["insert_pool"])
    for i, (g, w) in enumerate(zip(recs, want)):
        assert g == w, "region %d %s" % (i, regions[i])
    assert got["prev_end_out"] == regions[-1][1]
