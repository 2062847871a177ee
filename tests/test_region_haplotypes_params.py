"""Per-region parameters for the haplotype step (sk_region_haplotypes_params, sk_sync_region_params) and the whole chain of several samples on
one stream: per sample intake -> shared anchors -> synchronised walk -> params -> haplotypes -> alleles, against the models chained the
same way."""
import ctypes as C
import functools

import numpy as np
import pytest

from strelka_amd import capi
from tests import alleles_model as AL
from tests import anchor_model as A
from tests import haplotype_model as H
from tests import intake_model as M
from tests import region_haplotype_cases as R
from tests import sync_model as S
from tests import test_region_alleles as TA
from tests import test_region_haplotypes as T

pytestmark = pytest.mark.gpu


def _raw(c, regions, **kw):
    opt = capi.intake_options()
    opt.max_indel_size = c["max_indel_size"]
    return capi.region_haplotypes(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], regions, c["buf_begin"], c["buf_end"], c["ploidy"], opt=opt, raw=True, **kw)


def _scenario_case(sc, ploidy):
    regions = [(g["begin"], g["end"]) for g in sc["regions"] if g["ploidy"] == ploidy]
    return R.case(sc["reads"], regions, low=sc["low"], fwd=sc["fwd"], buf=(sc["buf_begin"], sc["buf_end"]), ploidy=ploidy, ref=sc["ref"], ref_offset=sc["ref_offset"],
                  max_indel_size=sc["max_indel_size"])


@pytest.mark.parametrize("name", sorted({s["name"].split("_")[0] for s in R.golden()}))
def test_uniform_records_give_the_existing_entrys_bytes(name):
    capi.init(0)
    n = 0
    for sc in R.golden():
        if sc["name"].split("_")[0] != name:
            continue
        for ploidy in (1, 2):
            c = _scenario_case(sc, ploidy)
            want = _raw(c, c["regions"])
            got = _raw(c, c["regions"], params=[(c["buf_begin"], c["buf_end"], ploidy)] * len(c["regions"]))
            for k in ("recs", "seq_pool", "support_pool", "query_off", "totals"):
                assert got[k].tobytes() == want[k].tobytes(), (sc["name"], ploidy, k)
            T._check_layout(got)
            n += len(c["regions"])
    assert n >= 2


@pytest.mark.parametrize("name", sorted({s["name"].split("_")[0] for s in R.golden()}))
def test_mixed_records_equal_one_call_of_the_existing_entry_per_region(name):
    capi.init(0)
    for sc in R.golden():
        if sc["name"].split("_")[0] != name:
            continue
        c = _scenario_case(sc, 2)
        regions = sorted({(g["begin"], g["end"]) for g in sc["regions"]})
        # ploidy 1 and 2 in turn; the buffer's range as recorded, ending at the region's end, ending one short of it (bypassed), beginning past its begin
        params = []
        for i, (b, e) in enumerate(regions):
            lo, hi = [(c["buf_begin"], c["buf_end"]), (c["buf_begin"], e), (c["buf_begin"], e - 1), (b + 1, c["buf_end"])][i % 4]
            params.append((lo, hi, 1 + i % 2))
        got = _raw(c, regions, params=params)
        T._check_layout(got)
        recs = capi.region_haplotype_records(got["recs"], got["seq_pool"], got["support_pool"])
        statuses = set()
        for i, (region, (lo, hi, ploidy)) in enumerate(zip(regions, params)):
            one = dict(c, buf_begin=lo, buf_end=hi, ploidy=ploidy)
            raw = _raw(one, [region])
            assert recs[i] == capi.region_haplotype_records(raw["recs"], raw["seq_pool"], raw["support_pool"])[0], (sc["name"], i, region)
            statuses.add(recs[i]["status"])
        if len(regions) >= 4:
            assert {H.COUNTED, H.BYPASSED} <= statuses


def _sync_regions(rows):
    a = np.zeros(len(rows), capi.SYNC_REGION_DTYPE)
    for i, (b, e, closed_at, ploidy) in enumerate(rows):
        a[i]["begin"], a[i]["end"], a[i]["closed_at"] = b, e, closed_at
        a[i]["ploidy"][:len(ploidy)] = ploidy
    return a


@pytest.mark.parametrize("n_regions", [0, 1, 255, 256, 257])
def test_params_from_the_synchronised_list(n_regions):
    capi.init(0)
    rows = [(100 + 20 * i, 110 + 20 * i, capi.SYNC_CLOSED_AT_CLEAR if i % 5 == 4 else 130 + 20 * i, [1 + i % 2, 2 - i % 2, 2]) for i in range(n_regions)]
    sync = _sync_regions(rows)
    for sample in (0, 1, 2):
        regions, params = capi.sync_region_params(sync, sample, 90, 7777)
        assert [tuple(int(x) for x in r) for r in regions] == [(b, e, at) for b, e, at, _ in rows]
        assert [tuple(int(x) for x in q) for q in params] == [(90, 7777 if at == capi.SYNC_CLOSED_AT_CLEAR else at, pl[sample], 0) for _, _, at, pl in rows]
    with pytest.raises(capi.StrelkaAmdError, match="sample"):
        capi.sync_region_params(sync, 8, 90)
    with pytest.raises(capi.StrelkaAmdError, match="sample"):
        capi.sync_region_params(sync, -1, 90)


def test_refused_records():
    import torch
    capi.init(0)
    L = capi.lib()
    c = R.case(R.plain(4), [(200, 210), (202, 212), (204, 214)])
    for bad in (0, 3):
        with pytest.raises(capi.StrelkaAmdError, match="sk_region_haplotypes_params: region 1: ploidy"):
            _raw(c, c["regions"], params=[(100, 500, 2), (100, 500, bad), (100, 500, 1)])
    assert [r["status"] for r in capi.region_haplotype_records(*[_raw(c, c["regions"], params=[(100, 500, 2)] * 3)[k] for k in ("recs", "seq_pool", "support_pool")])] == [H.COUNTED] * 3
    if L.sk_broker_client():
        return
    # the device entry: the sticky flag, and the region bypassed with nothing selected
    intake = capi.read_intake(c["ref"], c["ref_offset"], c["reads"], c["low"], 0, 0)
    d = T._dev_upload(c, 3, intake)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    regions = np.zeros(3, capi.ACTIVE_REGION_DTYPE)
    params = np.zeros(3, capi.REGION_PARAMS_DTYPE)
    for i, (b, e) in enumerate(c["regions"]):
        regions[i] = (b, e, 0)
        params[i] = (100, 500, (2, 3, 1)[i], 0)
    d_regions, d_params, d_n = dev(regions.view(np.int32)), dev(params.view(np.int32)), dev(np.array([3], np.int32))
    torch.cuda.synchronize()
    _launch_params(c, d, d_params, d_regions, d_n, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert L.sk_check_device_errors() != 0 and "ploidy" in capi.last_error()
    assert L.sk_check_device_errors() == 0
    recs = T._dev_records(d, 3)
    assert [r["status"] for r in recs] == [H.COUNTED, H.BYPASSED, H.COUNTED] and recs[1]["haps"] == []


def _launch_params(c, d, d_params, d_regions, d_n, stream):
    """sk_region_haplotypes_params_dev: only enqueues"""
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    t = d["t"]
    capi._check(capi.lib().sk_region_haplotypes_params_dev(p(d["ref"]), c["ref_offset"], len(c["ref"]), d["n"], p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]),
                                                           p(d["fwd"]), p(d["obs_off"]), p(d["obs"]), c["max_indel_size"], p(d_params), p(d_regions), p(d_n), d["region_cap"],
                                                           p(d["recs"]), p(d["seq"]), d["seq_cap"], p(d["support"]), d["support_cap"], p(d["query_off"]), p(d["totals"]),
                                                           p(d["scratch"]), d["scratch_bytes"], stream))


# ---- several samples, one stream ------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _samples():
    """three samples over one reference: the seeded window's reads; every second of them; every third, without the reads that carry an
    indel in the window's first half -- so the samples' detectors see different candidates"""
    c = R.seeded_window(n_reads=400, seed=9200)
    n = len(c["reads"])
    half = c["win_begin"] + c["n_pos"] // 2
    picks = [list(range(n)), list(range(1, n, 2)),
             [i for i in range(0, n, 3) if not (c["reads"][i]["pos"] < half and any(t in (R.IN, R.DE) for t, _ in c["reads"][i]["path"]))]]
    out = []
    for pick in picks:
        s = R.case([c["reads"][i] for i in pick], [], low=[c["low"][i] for i in pick], fwd=[c["fwd"][i] for i in pick], buf=(c["buf_begin"], c["buf_end"]), ref=c["ref"],
                   ref_offset=c["ref_offset"])
        s.update(win_begin=c["win_begin"], n_pos=c["n_pos"])
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def _model_of_the_chain(n_samples, max_hap_len):
    samples = _samples()[:n_samples]
    c0 = samples[0]
    win_begin, n_pos = c0["win_begin"], c0["n_pos"]
    intakes = [M.read_intake(c["ref"], c["ref_offset"], c["reads"], c["low"], win_begin, n_pos, c["max_indel_size"]) for c in samples]
    anchor, _ = A.ref_anchors(c0["ref"], c0["ref_offset"], win_begin + 1, None, win_begin, n_pos)
    depth = [[d for _, d in it["sites"]] for it in intakes]
    cand = [[int(x) for x in it["is_candidate"]] for it in intakes]
    plain, _, _ = S.sync_active_regions(win_begin, depth, cand, anchor)
    marks = [[] for _ in range(n_samples)]  # the last sample is haploid over every third region
    for g in plain[::3]:
        marks[-1] += [(g["begin"], 1), (g["end"] - 1, 1)]
    marks[-1] = sorted(set(marks[-1]))
    buf_end_at_clear = win_begin + n_pos + 1
    regions, state, region_id = S.sync_active_regions(win_begin, depth, cand, anchor, marks, 2, do_clear=True, buf_begin=[win_begin] * n_samples,
                                                      buf_end=[buf_end_at_clear] * n_samples)
    spans = [(g["begin"], g["end"]) for g in regions]
    per_sample = []
    for s, c in enumerate(samples):
        buf, _ = H.build_buffer(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], c["max_indel_size"])
        haps = [H.region_haplotypes(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], [span], win_begin,
                                    buf_end_at_clear if g["closed_at"] == S.CLOSED_AT_CLEAR else g["closed_at"], g["ploidy"][s], c["max_indel_size"], buf=buf)[0]
                for span, g in zip(spans, regions)]
        alleles, prev_end = AL.region_alleles(c["ref"], c["ref_offset"], spans, haps, c["max_indel_size"], max_hap_len, -1)
        per_sample.append(dict(haps=haps, alleles=alleles, prev_end=prev_end))
    return dict(intakes=intakes, anchor=anchor, marks=marks, regions=regions, state=state, region_id=region_id, per_sample=per_sample, buf_end_at_clear=buf_end_at_clear)


@pytest.mark.parametrize("n_samples", [2, 3])
def test_the_chain_of_several_samples_on_one_stream(n_samples):
    """per sample sk_read_intake_dev -> sk_ref_anchors_dev -> sk_sync_active_regions_dev -> per sample sk_sync_region_params_dev ->
    sk_region_haplotypes_params_dev -> sk_region_alleles_dev, one stream, no host copy in between"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    max_hap_len = 128
    samples = _samples()[:n_samples]
    m = _model_of_the_chain(n_samples, max_hap_len)
    regions = m["regions"]
    assert len(regions) >= 6 and any(bin(g["sample_mask"]).count("1") >= 2 for g in regions) and any(len(set(g["ploidy"])) > 1 for g in regions)
    assert any(g["sample_mask"] != (1 << n_samples) - 1 for g in regions)  # the samples do not all see the same
    assert any(r["n_alt"] >= 1 for ps in m["per_sample"] for r in ps["alleles"])
    c0 = samples[0]
    win_begin, n_pos = c0["win_begin"], c0["n_pos"]
    region_cap = capi.sync_regions_bound(n_pos)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    d_sites = torch.zeros(n_samples * n_pos, dtype=torch.int64, device="cuda")
    d_cand = torch.zeros(n_samples * n_pos, dtype=torch.uint8, device="cuda")
    d_anchor = torch.zeros(n_pos, dtype=torch.uint8, device="cuda")
    mark_off, marks = capi.pack_ploidy_marks(m["marks"], n_samples)
    d_mark_off, d_marks = dev(mark_off), dev(marks.view(np.int32))
    d_state = dev(capi.sync_state_initial().view(np.int32))
    d_sync = torch.zeros(region_cap * 8, dtype=torch.int32, device="cuda")
    d_n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    d_id = torch.full((n_pos,), 7, dtype=torch.int32, device="cuda")
    allele_cap, insert_cap = capi.region_alleles_bounds(region_cap, max_hap_len)
    a_scratch_bytes = L.sk_region_alleles_scratch_bytes(region_cap, max_hap_len)
    per = []
    for c in samples:
        n = len(c["reads"])
        d = T._dev_upload(c, region_cap)
        cap = capi.read_intake_obs_bound(d["n_segs"])
        d.update(reads=torch.zeros(n * 16, dtype=torch.uint8, device="cuda"), obs_off=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                 obs=torch.zeros(cap * 32, dtype=torch.uint8, device="cuda"), obs_cap=cap, intake_scratch_bytes=L.sk_read_intake_scratch_bytes(n, d["n_segs"], n_pos),
                 regions=torch.zeros(region_cap * 3, dtype=torch.int32, device="cuda"), params=torch.zeros(region_cap * 4, dtype=torch.int32, device="cuda"),
                 a=dict(recs=torch.full((region_cap * 72,), 0x5a, dtype=torch.uint8, device="cuda"), alleles=torch.zeros(allele_cap * 56, dtype=torch.uint8, device="cuda"),
                        ins=torch.zeros(insert_cap, dtype=torch.uint8, device="cuda"), totals=torch.full((2,), -1, dtype=torch.int64, device="cuda"),
                        prev=torch.full((1,), -7, dtype=torch.int32, device="cuda")),
                 a_scratch=torch.zeros(a_scratch_bytes, dtype=torch.uint8, device="cuda"))
        d["intake_scratch"] = torch.zeros(d["intake_scratch_bytes"], dtype=torch.uint8, device="cuda")
        per.append(d)
    opt = capi.intake_options()
    b = np.array([win_begin] * n_samples, np.int32)
    e = np.array([m["buf_end_at_clear"]] * n_samples, np.int32)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for s, (c, d) in enumerate(zip(samples, per)):
        t = d["t"]
        capi._check(L.sk_read_intake_dev(p(d["ref"]), c["ref_offset"], len(c["ref"]), d["n"], p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]), C.byref(opt),
                                         win_begin, n_pos, p(d["reads"]), p(d["obs_off"]), p(d["obs"]), d["obs_cap"], p(d_sites[s * n_pos:]), p(d_cand[s * n_pos:]),
                                         p(d["intake_scratch"]), d["intake_scratch_bytes"], st))
    capi._check(L.sk_ref_anchors_dev(p(per[0]["ref"]), c0["ref_offset"], len(c0["ref"]), win_begin + 1, None, win_begin, n_pos, p(d_anchor), 0, None, None, st))
    capi._check(L.sk_sync_active_regions_dev(n_samples, win_begin, n_pos, p(d_sites), p(d_cand), p(d_anchor), p(d_mark_off), p(d_marks), 2, p(d_state), p(d_state), 1,
                                             capi._p(b), capi._p(e), p(d_sync), region_cap, p(d_n), p(d_id), st))
    for s, (c, d) in enumerate(zip(samples, per)):
        capi._check(L.sk_sync_region_params_dev(p(d_sync), p(d_n), region_cap, s, win_begin, m["buf_end_at_clear"], p(d["regions"]), p(d["params"]), st))
        _launch_params(c, d, d["params"], d["regions"], d_n, st)
        a = d["a"]
        capi._check(L.sk_region_alleles_dev(p(d["ref"]), c["ref_offset"], len(c["ref"]), p(d["regions"]), p(d_n), region_cap, p(d["recs"]), p(d["seq"]), d["seq_cap"],
                                            c["max_indel_size"], max_hap_len, -1, p(a["recs"]), p(a["alleles"]), allele_cap, p(a["ins"]), insert_cap, p(a["totals"]),
                                            p(a["prev"]), p(d["a_scratch"]), a_scratch_bytes, st))
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    n_regions = int(d_n.cpu()[0])
    assert n_regions == len(regions)
    got = d_sync.cpu().numpy()[:n_regions * 8].view(capi.SYNC_REGION_DTYPE)
    for g, w in zip(got, regions):
        assert (int(g["begin"]), int(g["end"]), int(g["closed_at"]), int(g["prev_end"]), g["ploidy"][:n_samples].tolist(), int(g["sample_mask"])) == \
            (w["begin"], w["end"], w["closed_at"], w["prev_end"], w["ploidy"], w["sample_mask"])
    assert d_id.cpu().tolist() == m["region_id"]
    assert d_anchor.cpu().tolist() == m["anchor"]
    state = capi.sync_state_dict(d_state.cpu().numpy().view(capi.SYNC_STATE_DTYPE), n_samples)
    assert state == dict(m["state"], samples=m["state"]["samples"][:n_samples])
    for s, (d, want) in enumerate(zip(per, m["per_sample"])):
        assert d_cand[s * n_pos:(s + 1) * n_pos].cpu().numpy().astype(bool).tolist() == [bool(x) for x in m["intakes"][s]["is_candidate"]]
        haps = T._dev_records(d, n_regions)
        for i, (g, w) in enumerate(zip(haps, want["haps"])):
            assert g == w, "sample %d region %d" % (s, i)
        raw = TA._dev_raw(d["a"], n_regions)
        TA._check_layout(raw)
        recs = capi.region_allele_records(raw["recs"], raw["alleles"], raw["insert_pool"])
        for i, (g, w) in enumerate(zip(recs, want["alleles"])):
            assert g == w, "sample %d region %d" % (s, i)
            assert g["prev_end"] == regions[i]["prev_end"]  # what the alleles step derives is what the synchroniser recorded
        assert raw["prev_end_out"] == want["prev_end"] == regions[-1]["end"]
