"""Region haplotypes on the device (sk_region_haplotypes, csrc/region_haplotypes.hip): every field of every output equals the loop
model (tests/haplotype_model.py, itself pinned to vectors recorded from the reference by tests/test_region_haplotypes_model.py)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from strelka_amd import capi
from tests import haplotype_model as H
from tests import intake_model as M
from tests import region_haplotype_cases as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS, IN, DE, SC, HC = R.MS, R.IN, R.DE, R.SC, R.HC


def _check_layout(raw):
    """the pools lie back to back in region order, query_off names every selected haplotype's bytes, totals count them"""
    at_seq = at_sup = k = 0
    for r in raw["recs"]:
        for j in range(capi.HAP_MAX_SELECTED):
            h = r["hap"][j]
            if j >= int(r["n_selected"]):
                assert h.tobytes() == bytes(32)
                continue
            assert (int(h["seq_off"]), int(h["support_off"])) == (at_seq, at_sup) and int(raw["query_off"][k]) == at_seq
            at_seq += int(h["seq_len"])
            at_sup += int(h["count"])
            k += 1
        assert int(r["pad"]) == 0
    assert raw["totals"].tolist() == [k, at_seq, at_sup] and int(raw["query_off"][k]) == at_seq and len(raw["query_off"]) == k + 1


def _run(c, what=""):
    """device against model -> the model's records"""
    capi.init(0)
    want = R.model(c)
    opt = capi.intake_options()
    opt.max_indel_size = c["max_indel_size"]
    raw = capi.region_haplotypes(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], c["regions"], c["buf_begin"], c["buf_end"], c["ploidy"], opt=opt, raw=True)
    got = capi.region_haplotype_records(raw["recs"], raw["seq_pool"], raw["support_pool"])
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s region %d %s" % (what, i, c["regions"][i])
    _check_layout(raw)
    return want


def _long_reads():
    """reads of 300 bases over 120..419: the reference, three other haplotypes, an insertion, a deletion"""
    reads = R.plain(6, pos=120, length=300)
    reads += R.plain(4, subs={200: None, 262: None}, pos=120, length=300)
    reads += R.plain(3, subs={263: None}, pos=120, length=300)
    reads += R.plain(3, subs={264: None, 399: None}, pos=120, length=300)
    reads += [R.read(120, [(MS, 100), (IN, 3), (MS, 197)], ins=["GAT"])] * 3
    reads += [R.read(120, [(MS, 143), (DE, 2), (MS, 157)])] * 3
    return reads


def test_region_lengths_1_2_63_64_65_250_and_251():
    c = R.case(_long_reads(), [(200, 201), (200, 202), (200, 263), (200, 264), (200, 265), (150, 400), (150, 401), (263, 265), (219, 220)])
    want = _run(c, "lengths")
    assert [r["status"] for r in want] == [H.COUNTED] * 6 + [H.BYPASSED] + [H.COUNTED] * 2
    assert [len(r["haps"]) for r in want] == [2, 2, 2, 2, 2, 2, 0, 3, 2] and len(want[5]["haps"][0]["seq"]) == 250 and len(want[8]["haps"][1]["seq"]) == 4
    c["ploidy"] = 1
    _run(c, "lengths, haploid")


def test_regions_clipped_by_the_buffers_range():
    reads = _long_reads()
    regions = [(150, 160), (149, 160), (390, 400), (390, 401), (150, 400)]
    want = _run(R.case(reads, regions, buf=(150, 400)), "clipped")
    assert [r["status"] for r in want] == [H.COUNTED, H.BYPASSED, H.COUNTED, H.BYPASSED, H.COUNTED]
    want = _run(R.case(reads, regions, buf=(151, 399)), "clipped, narrower")
    assert [r["status"] for r in want] == [H.BYPASSED] * 5


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65])
def test_registered_read_counts(n):
    reads = [R.read(300, [(MS, 40)])] * 2 + R.plain((n + 1) // 2) + R.plain(n // 2, subs={205: None})
    want = _run(R.case(reads, [(200, 210), (203, 206)]), "%d reads" % n)
    assert want[0]["n_reads_aligned"] == n and want[0]["status"] == (H.NO_READS if n == 0 else H.COUNTED)
    assert len(want[0]["haps"]) == (0 if n < 5 else 2)  # (two and one read of a haplotype do not reach MinHaplotypeCount)


def test_the_kinds_of_read():
    """soft clips, N, '=', low MAPQ, swaps, breakpoints, partial reads, hard clips, edge indels, insertions over mismatches and at
    begin - 1, deletions at the last position, reads hanging off the reference segment -- crafted here, and in the recorded scenes"""
    reads = R.plain(4) + R.plain(3, subs={205: None})
    reads += [R.read(206, [(SC, 5), (MS, 40)]), R.read(170, [(MS, 35), (SC, 4)]), R.read(180, [(MS, 60)], subs={203: "N"}), R.read(180, [(MS, 60)], subs={204: "="})]
    reads += [R.read(180, [(MS, 22), (IN, 2), (DE, 3), (MS, 30)]), R.read(140, [(MS, 62), (DE, 50), (MS, 20)]), R.read(204, [(MS, 40)]), R.read(150, [(MS, 55)])]
    reads += [R.read(180, [(HC, 3), (MS, 60), (HC, 2)]), R.read(190, [(IN, 2), (MS, 40)]), R.read(96, [(MS, 30)])]
    reads += [R.read(180, [(MS, 25), (IN, 3), (MS, 30)], subs={204: None}, ins=["ACA"])] * 3 + [R.read(180, [(MS, 25), (IN, 3), (MS, 30)], ins=["ACA"])] * 3
    reads += [R.read(180, [(MS, 20), (IN, 2), (MS, 35)], ins=["GT"])] * 3 + [R.read(180, [(MS, 31), (DE, 1), (MS, 30)])] * 3
    reads += [R.read(180, [(MS, 25), (IN, 2), (MS, 30)], ins=["NA"])]
    low = [0] * len(reads)
    low[5] = 1
    regions = [(200, 212), (210, 220), (205, 206), (202, 205), (199, 212), (96, 104), (100, 104), (204, 205)]
    c = R.case(reads, regions, low=low)
    _run(c, "kinds")
    c["ploidy"] = 1
    _run(c, "kinds, haploid")


def test_index_spread_of_999_and_1000():
    assert _run(R.spread_case(999), "spread 999")[0]["status"] == H.COUNTED
    rec = _run(R.spread_case(1000), "spread 1000")[0]
    assert (rec["status"], rec["reason"]) == (H.DECLINED, H.DECLINE_READ_INDEX_SPREAD)


def test_read_span_of_999_and_1000():
    for length, status in ((900, H.COUNTED), (901, H.DECLINED)):
        c = R.case(R.plain(3) + [R.read(150, [(MS, 55), (DE, length), (MS, 45)])], [(200, 204)], max_indel_size=1000)
        rec = _run(c, "deletion of %d" % length)[0]
        assert rec["status"] == status and rec["reason"] == (H.DECLINE_READ_SPAN if status == H.DECLINED else 0)


def test_16_and_17_qualifying_groups():
    want = _run(R.groups_case(16), "16 groups")[0]
    assert want["status"] == H.COUNTED
    rec = _run(R.groups_case(17), "17 groups")[0]
    assert (rec["status"], rec["reason"]) == (H.DECLINED, H.DECLINE_GROUPS)
    # 17 groups of which 16 reach MinHaplotypeCount
    c = R.groups_case(17)
    c["reads"] = c["reads"][:-1]
    c["fwd"], c["low"] = c["fwd"][:-1], c["low"][:-1]
    assert _run(c, "16 of 17")[0]["status"] == H.COUNTED


@pytest.mark.parametrize("n_regions", [0, 1, 2, 65])
def test_region_counts(n_regions):
    reads = _long_reads()
    regions = [(150 + 3 * i, 150 + 3 * i + 1 + (i % 7)) for i in range(n_regions)]
    want = _run(R.case(reads, regions), "%d regions" % n_regions)
    assert len(want) == n_regions


@pytest.mark.parametrize("name", sorted({s["name"].split("_")[0] for s in R.golden()}))
def test_recorded_vectors(name):
    for sc in R.golden():
        if sc["name"].split("_")[0] != name:
            continue
        for ploidy in (1, 2):
            regions = [g for g in sc["regions"] if g["ploidy"] == ploidy]
            c = R.case(sc["reads"], [(g["begin"], g["end"]) for g in regions], low=sc["low"], fwd=sc["fwd"], buf=(sc["buf_begin"], sc["buf_end"]), ploidy=ploidy,
                       ref=sc["ref"], ref_offset=sc["ref_offset"], max_indel_size=sc["max_indel_size"])
            want = _run(c, "%s ploidy %d" % (sc["name"], ploidy))
            for w, g in zip(want, regions):  # ... and the recorded fields themselves
                assert [dict(seq=h["seq"], support=h["support"]) for h in w["haps"]] == g["selected"]
                if w["status"] != H.BYPASSED:
                    assert w["n_reads_aligned"] == g["n_reads_aligned"]


def test_narrow_hash_is_decided_by_the_bytes(monkeypatch):
    """with the hash cut to 4 bits most of 40 distinct haplotypes collide: the classes still come from the bytes"""
    reads = []
    for g in range(40):
        reads += R.plain(1 + g % 5, subs={201 + k: None for k in range(6) if (g + 1) >> k & 1})
    order = np.random.default_rng(77).permutation(len(reads))
    c = R.case([reads[i] for i in order], [(200, 210), (201, 204)])
    monkeypatch.setenv("SK_HAP_TEST_HASH_BITS", "4")
    want = _run(c, "4-bit hash")
    assert want[0]["status"] == H.DECLINED and want[0]["reason"] == H.DECLINE_GROUPS and want[1]["status"] == H.COUNTED
    c["regions"] = [(203, 210), (204, 207)]
    assert [r["status"] for r in _run(c, "4-bit hash, fewer groups")] == [H.COUNTED, H.COUNTED]
    monkeypatch.setenv("SK_HAP_TEST_HASH_BITS", "1")
    _run(c, "1-bit hash")


def test_refused_inputs():
    capi.init(0)
    reads = R.plain(3)
    ok = R.case(reads, [(200, 210)])

    def call(c, **kw):
        return capi.region_haplotypes(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], c["regions"], c["buf_begin"], c["buf_end"], kw.get("ploidy", 2))
    for ploidy in (0, 3):
        with pytest.raises(capi.StrelkaAmdError, match="ploidy"):
            call(ok, ploidy=ploidy)
    with pytest.raises(capi.StrelkaAmdError, match="end <= begin"):
        call(R.case(reads, [(200, 210), (210, 210)]))
    def call_with_no_observations(c):
        empty = dict(obs_off=np.zeros(len(c["reads"]) + 1, np.int64), obs=np.zeros(0, capi.INTAKE_OBS_DTYPE))
        return capi.region_haplotypes(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], c["regions"], c["buf_begin"], c["buf_end"], 2, intake=empty)
    with pytest.raises(capi.StrelkaAmdError, match="sk_region_haplotypes: read 3: the path's read length"):
        call_with_no_observations(R.case(reads + [dict(code=M.encode("ACGT"), pos=200, path=[(MS, 5)])], [(200, 210)]))
    with pytest.raises(capi.StrelkaAmdError, match="sk_region_haplotypes: read 0: longer than SK_PILEUP_MAX_READ_LEN"):
        call_with_no_observations(R.case([dict(code=M.encode("A" * 1025), pos=200, path=[(MS, 1025)])], [(200, 210)]))
    L = capi.lib()
    assert L.sk_region_haplotypes_seq_bound(-1) == -1 and L.sk_region_haplotypes_support_bound(-1, 1) == -1
    assert capi.region_haplotypes_bounds(5000, 7) == (7 * 3 * 1024, 7 * 1000) and capi.region_haplotypes_bounds(12, 7) == (7 * 3 * 1024, 7 * 12)
    # a pool below its bound
    z = np.zeros(16, np.int64)
    one = np.zeros(1, capi.ACTIVE_REGION_DTYPE)
    one[0] = (0, 4, 0)
    for seq_cap, support_cap, which in ((3071, 0, "seq_cap"), (3072, -1, "negative size")):
        rc = L.sk_region_haplotypes(b"ACGT", 0, 4, 0, None, None, None, None, None, None, None, None, None, None, 49, 0, 4, 2, capi._p(one), 1,
                                    capi._p(np.zeros(1, capi.REGION_HAPLOTYPES_DTYPE)), capi._p(np.zeros(3072, np.uint8)), seq_cap, capi._p(np.zeros(8, np.int32)), support_cap,
                                    capi._p(z), capi._p(z))
        assert rc != 0 and which in capi.last_error()
    assert call(ok)[0]["status"] == H.COUNTED  # and the library goes on working


def _dev_upload(c, region_cap, intake=None):
    """the reads of a case on the device (their bases at an odd address), the observations when given as host arrays, and room for the
    outputs of sk_region_haplotypes_dev -> dict of device tensors"""
    import torch
    L = capi.lib()
    n = len(c["reads"])
    read_off, code, path_off, n_seg, path, pos = capi.pack_reads(c["reads"])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    holder = torch.zeros(len(code) + 8, dtype=torch.uint8, device="cuda")
    d_code = holder[1:1 + len(code)]
    d_code.copy_(dev(code))
    assert d_code.data_ptr() % 2 == 1
    d = dict(ref=dev(np.frombuffer(c["ref"].encode(), np.uint8).copy()), holder=holder, n=n, n_segs=int(path_off[-1]), region_cap=region_cap,
             t=[dev(read_off), d_code, dev(path_off), dev(n_seg), dev(path.view(np.uint32)), dev(pos), dev(np.array(list(c["low"]) + [0], np.uint8))],
             fwd=dev(np.array(list(c["fwd"]) + [0], np.uint8)))
    if intake is not None:
        d["obs_off"] = dev(np.ascontiguousarray(intake["obs_off"], np.int64))
        d["obs"] = dev(np.ascontiguousarray(intake["obs"], capi.INTAKE_OBS_DTYPE).view(np.uint8)) if len(intake["obs"]) else None
    d["seq_cap"], d["support_cap"] = capi.region_haplotypes_bounds(n, region_cap)
    d["recs"] = torch.full((max(region_cap, 1) * 120,), 0x5a, dtype=torch.uint8, device="cuda")
    d["seq"] = torch.zeros(max(d["seq_cap"], 1), dtype=torch.uint8, device="cuda")
    d["support"] = torch.zeros(max(d["support_cap"], 1), dtype=torch.int32, device="cuda")
    d["query_off"] = torch.full((3 * region_cap + 1,), -1, dtype=torch.int64, device="cuda")
    d["totals"] = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    d["scratch_bytes"] = L.sk_region_haplotypes_scratch_bytes(n, region_cap, d["seq_cap"], d["support_cap"])
    d["scratch"] = torch.zeros(d["scratch_bytes"], dtype=torch.uint8, device="cuda")
    return d


def _dev_launch(c, d, d_regions, d_n, stream):
    """sk_region_haplotypes_dev: only enqueues"""
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    t = d["t"]
    capi._check(capi.lib().sk_region_haplotypes_dev(p(d["ref"]), c["ref_offset"], len(c["ref"]), d["n"], p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]),
                                                    p(d["fwd"]), p(d["obs_off"]), p(d["obs"]), c["max_indel_size"], c["buf_begin"], c["buf_end"], c["ploidy"], p(d_regions),
                                                    p(d_n), d["region_cap"], p(d["recs"]), p(d["seq"]), d["seq_cap"], p(d["support"]), d["support_cap"], p(d["query_off"]),
                                                    p(d["totals"]), p(d["scratch"]), d["scratch_bytes"], stream))


def _dev_call(c, intake, d_regions, d_n, region_cap):
    import torch
    d = _dev_upload(c, region_cap, intake)
    torch.cuda.synchronize()
    _dev_launch(c, d, d_regions, d_n, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return d


def _dev_records(out, n_regions):
    recs = out["recs"].cpu().numpy()[:n_regions * 120].view(capi.REGION_HAPLOTYPES_DTYPE)
    totals = out["totals"].cpu().numpy()
    raw = dict(recs=recs, seq_pool=out["seq"].cpu().numpy()[:int(totals[1])], support_pool=out["support"].cpu().numpy()[:int(totals[2])],
               query_off=out["query_off"].cpu().numpy()[:int(totals[0]) + 1], totals=totals)
    _check_layout(raw)
    return capi.region_haplotype_records(recs, raw["seq_pool"], raw["support_pool"])


def test_device_entry_flags_an_empty_region_and_leaves_slots_past_n_regions_alone():
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    c = R.case(R.plain(4) + R.plain(3, subs={205: None}), [(200, 210), (203, 206), (220, 230)])
    intake = M.read_intake(c["ref"], c["ref_offset"], c["reads"], c["low"], 0, 0)
    intake = dict(obs_off=intake["obs_off"], obs=np.zeros(0, capi.INTAKE_OBS_DTYPE))
    regions = np.zeros(5, capi.ACTIVE_REGION_DTYPE)
    for i, (b, e) in enumerate(c["regions"]):
        regions[i] = (b, e, 0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    # n_regions = 2 below region_cap = 5: the third region is not looked at
    out = _dev_call(c, intake, dev(regions.view(np.int32)), dev(np.array([2], np.int32)), 5)
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    assert _dev_records(out, 2) == R.model(c)[:2]
    assert out["recs"].cpu().numpy()[2 * 120:].tolist() == [0x5a] * (3 * 120)
    # an empty region: the host entry refuses it, the device entry raises the sticky flag and bypasses it
    regions[1] = (206, 206, 0)
    out = _dev_call(c, intake, dev(regions.view(np.int32)), dev(np.array([3], np.int32)), 5)
    torch.cuda.synchronize()
    assert L.sk_check_device_errors() != 0 and "sk_region_haplotypes_dev" in capi.last_error()
    assert L.sk_check_device_errors() == 0
    got = _dev_records(out, 3)
    want = R.model(c)
    assert got[0] == want[0] and got[2] == want[2] and got[1]["status"] == H.BYPASSED and got[1]["haps"] == []
    # refused on the host side of the device entry: a pool below its bound, a bad ploidy
    c2 = dict(c, ploidy=3)
    with pytest.raises(capi.StrelkaAmdError, match="ploidy"):
        _dev_call(c2, intake, dev(regions.view(np.int32)), dev(np.array([1], np.int32)), 5)


def test_four_calls_on_one_stream_on_the_seeded_window():
    """sk_read_intake_dev -> sk_ref_anchors_dev -> sk_active_regions_dev -> sk_region_haplotypes_dev on one stream, no host copy in
    between, the read bases at an odd address"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    c, intake, anchor, regions, want = R.seeded_window_model()
    assert sum(1 for r in want if r["status"] == H.COUNTED and len(r["haps"]) >= 2) * 2 >= len(want) and not any(r["status"] == H.DECLINED for r in want)
    capi.init(0)
    L = capi.lib()
    n = len(c["reads"])
    win_begin, n_pos = c["win_begin"], c["n_pos"]
    region_cap = capi.active_regions_bound(n_pos)
    d = _dev_upload(c, region_cap)
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
    opt = capi.intake_options()
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi._check(L.sk_read_intake_dev(p(d_ref), c["ref_offset"], len(c["ref"]), n, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]), C.byref(opt),
                                     win_begin, n_pos, p(d_reads), p(d_obs_off), p(d_obs), cap, p(d_sites), p(d_cand), p(d_scratch), scratch_bytes, st))
    capi._check(L.sk_ref_anchors_dev(p(d_ref), c["ref_offset"], len(c["ref"]), win_begin + 1, None, win_begin, n_pos, p(d_anchor), 0, None, None, st))
    capi._check(L.sk_active_regions_dev(win_begin, n_pos, p(d_sites), p(d_cand), p(d_anchor), p(d_state_in), p(d_state_out), p(d_regions), region_cap, p(d_n), st))
    d["obs_off"], d["obs"] = d_obs_off, d_obs
    _dev_launch(c, d, d_regions, d_n, st)
    out = d
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    assert int(d_n.cpu()[0]) == len(regions)
    assert [tuple(int(x) for x in r) for r in d_regions.cpu().numpy().view(capi.ACTIVE_REGION_DTYPE)[:len(regions)]] == regions
    got = _dev_records(out, len(regions))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "region %d %s" % (i, regions[i])
    # the host entries, chained by the caller, give the same records
    assert _run(c, "host chain") == want


def _host_digest():
    sc = next(s for s in R.golden() if s["name"] == "indels")
    regions = [(g["begin"], g["end"]) for g in sc["regions"] if g["ploidy"] == 2]
    raw = capi.region_haplotypes(sc["ref"], sc["ref_offset"], sc["reads"], sc["low"], sc["fwd"], regions, sc["buf_begin"], sc["buf_end"], 2, raw=True)
    data = raw["recs"].tobytes() + raw["seq_pool"].tobytes() + raw["support_pool"].tobytes() + raw["query_off"].tobytes() + raw["totals"].tobytes()
    return data, int(raw["totals"][0])


BROKER_CLIENT = r'''
import hashlib, json, sys
sys.path.insert(0, %r)
from strelka_amd import capi
from tests import test_region_haplotypes as T
capi.init(0)
data, n = T._host_digest()
print(json.dumps(dict(client=capi.lib().sk_broker_client(), digest=hashlib.sha256(data).hexdigest(), n_haplotypes=n)))
'''


def test_through_the_broker(tmp_path):
    capi.init(0)
    direct, n = _host_digest()
    env = dict(os.environ, STRELKA_AMD_BROKER="1", STRELKA_AMD_BROKER_SOCKET="sktest_" + uuid.uuid4().hex[:12], STRELKA_AMD_BROKER_LOG=str(tmp_path / "broker.log"),
               STRELKA_AMD_BROKER_IDLE_S="2")
    p = subprocess.run([sys.executable, "-c", BROKER_CLIENT % REPO], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    res = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert res["client"] == 1
    assert res["n_haplotypes"] == n >= 8
    assert res["digest"] == hashlib.sha256(direct).hexdigest()
