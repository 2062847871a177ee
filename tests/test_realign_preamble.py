"""The realignment preamble on the device (sk_realign_preamble; csrc/realign_preamble.hip): records, source, status bytes, totals and preamble_consulted
equal, with zero differing bytes, what the same core gives on the host (sk_debug_realign_preamble_host, itself held to the job's own preamble by
tests/test_realign_preamble_host.py) -- through the host entry, the _dev entry, and behind sk_indel_table_dev -> sk_read_depth_dev ->
sk_indel_candidates_dev -> sk_realign_gate_dev on one stream.  Then what the records are for: a job fed by sk_realign_job_add_reads_prepared with the device's
records gives every read the result a job fed by plain sk_realign_job_add_reads gives it.

The scenes are the 82 recorded gate scenes and the crafted windows of tests/realign_preamble_cases.py: 0 / 1 / 40 / 41 keys in one range (one turn of 64
lanes; the capacity), observed lists of 0 / 1 / 64 / 65, paths of 1 / 47 / 51 segments, one and two samples, reads that leave at every status."""
import ctypes as C

import numpy as np
import pytest

from strelka_amd import capi
from tests import indel_candidates_cases as K
from tests import indel_candidates_model as CM
from tests import realign_gate_model as GM
from tests import realign_preamble_cases as P

pytestmark = pytest.mark.gpu

SLACK = 2


@pytest.fixture(scope="module")
def scenes():
    """every scene once: (scene, the model's gate outputs, insert pool, the core's result on the host)"""
    capi.init(0)
    out = []
    for sc in P.all_scenes():
        gate, ins, _ = P.model_gate(sc)
        out.append((sc, gate, ins, P.preamble(sc, True, gate, ins)))
    return out


def _same(sc, got, want, slack, record_cap=None, key_cap=None):
    """a device result over rooms with `slack` canary elements against the host's; zero differing bytes"""
    n_rec, nk = want["totals"][0], len(sc["keys"])
    record_cap = len(want["records"]) if record_cap is None else record_cap
    key_cap = nk if key_cap is None else key_cap
    assert got["totals"] == want["totals"], sc["name"]
    assert got["records"][:n_rec].tobytes() == want["records"][:n_rec].tobytes(), sc["name"]
    assert got["source"][:n_rec].tobytes() == want["source"][:n_rec].tobytes(), sc["name"]
    assert not got["records"][n_rec:record_cap].view(np.uint8).any() and not got["source"][n_rec:record_cap].view(np.uint8).any(), sc["name"]
    assert (got["records"][record_cap:].view(np.uint8) == 0x5a).all() and (got["source"][record_cap:].view(np.uint8) == 0x5a).all() and len(got["records"]) == record_cap + slack
    assert (got["consulted"][:nk] == want["consulted"][:nk]).all() and not got["consulted"][nk:key_cap].any() and (got["consulted"][key_cap:] == 0x5a).all(), sc["name"]
    for s, sm in enumerate(sc["samples"]):
        n = len(sm["reads"])
        assert (got["status"][s][:n] == want["status"][s][:n]).all() and (got["status"][s][n:] == 0x5a).all(), (sc["name"], s)


def test_host_entry_equals_the_core_on_every_scene(scenes):
    for sc, gate, ins, want in scenes:
        _same(sc, P.preamble(sc, False, gate, ins, slack=SLACK), want, SLACK)


def _dev(sc, gate, ins, key_cap=None, record_cap=None, n_keys=None, mutate=None):
    """sk_realign_preamble_dev on uploaded arrays -> capi.realign_preamble's form over all of the rooms, canaries of SLACK elements behind every output"""
    import torch
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
    n_samples, nk = len(sc["samples"]), len(sc["keys"])
    key_cap = nk + 3 if key_cap is None else key_cap
    n_pass = sum(int((g["reads"]["status"][:len(sm["reads"])] == capi.RGATE_PASS).sum()) for g, sm in zip(gate["samples"], sc["samples"]))
    record_cap = n_pass + 1 if record_cap is None else record_cap
    ps, pp = P.packed(sc)
    gs = [dict(reads=g["reads"].copy(), observed_off=g["observed_off"].copy(), observed=g["observed"].copy(), observed_cap=g["observed_cap"]) for g in gate["samples"]]
    if mutate:
        mutate(ps, pp, gs)
    room = lambda n, itemsize: torch.full(((max(n, 0) + SLACK) * itemsize,), 0x5a, dtype=torch.uint8, device="cuda")
    keep, a_in, a_gate, a_pre, status = [], [], [], [], []
    for p, q, g in zip(ps, pp, gs):
        d = {f: dev(p[f]) for f in ("pos", "path_off", "n_seg", "path", "read_len", "realign_begin", "realign_end")}
        e = dict(reads=dev(g["reads"]), observed_off=dev(g["observed_off"]), observed=dev(g["observed"]), read_code=dev(q["read_code"]), read_off=dev(q["read_off"]),
                 fwd=dev(q["is_fwd_strand"]), status=room(p["n_reads"], 1))
        keep.append((d, e))
        status.append(e["status"])
        a_in.append(capi.realign_gate_sample_struct(dict(p, align_id=None, **d), ptr=lambda x: x.data_ptr()))
        a_gate.append(capi.RealignGateSampleOut(e["reads"].data_ptr(), e["observed_off"].data_ptr(), e["observed"].data_ptr(), g["observed_cap"]))
        a_pre.append(capi.RealignPreambleSample(e["read_code"].data_ptr(), e["read_off"].data_ptr(), q["code_cap"], e["fwd"].data_ptr(), e["status"].data_ptr()))
    arr_in, arr_gate, arr_pre = (capi.RealignGateSample * n_samples)(*a_in), (capi.RealignGateSampleOut * n_samples)(*a_gate), (capi.RealignPreambleSample * n_samples)(*a_pre)
    keys = np.zeros(key_cap + 1, capi.REALIGN_GATE_KEY_DTYPE)
    keys[:min(nk, key_cap)] = gate["keys"][:key_cap]
    t = dict(keys=dev(keys), totals=dev(np.array([nk if n_keys is None else n_keys, 0, 0, 0], np.int64)), ins=dev(np.concatenate([ins, np.zeros(1, np.uint8)])),
             ref=dev(np.frombuffer(sc["ref"].encode() + b"\0", np.uint8)))
    records, source, consulted = room(record_cap, 784), room(record_cap, 8), room(key_cap, 1)
    totals = torch.full((capi.RPRE_N_TOTALS,), -1, dtype=torch.int64, device="cuda")
    scratch_bytes = capi.realign_preamble_scratch_bytes(n_samples, key_cap, record_cap)
    scratch = torch.full((scratch_bytes,), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    capi.realign_preamble_dev(n_samples, C.addressof(arr_in), C.addressof(arr_gate), C.addressof(arr_pre), t["keys"].data_ptr(), t["totals"].data_ptr(), key_cap, t["ins"].data_ptr(),
                              len(ins), t["ref"].data_ptr(), sc["ref_offset"], len(sc["ref"]), sc["max_indel_size"], records.data_ptr(), source.data_ptr(), record_cap,
                              consulted.data_ptr(), totals.data_ptr(), scratch.data_ptr(), scratch_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(records=records.cpu().numpy().view(capi.REALIGN_PREPARED_READ_DTYPE), source=source.cpu().numpy().view(capi.REALIGN_PREPARED_SOURCE_DTYPE),
                consulted=consulted.cpu().numpy(), totals=totals.cpu().numpy().tolist(), status=[s.cpu().numpy() for s in status]), key_cap, record_cap


def _needs_own_context():
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")


def test_dev_entry_equals_the_core_on_every_scene(scenes):
    _needs_own_context()
    for sc, gate, ins, want in scenes:
        got, key_cap, record_cap = _dev(sc, gate, ins)
        capi._check(capi.lib().sk_check_device_errors())
        _same(sc, got, want, SLACK, record_cap, key_cap)
    sc, gate, ins, want = next(x for x in scenes if x[0]["name"] == "two_samples")
    got, key_cap, record_cap = _dev(sc, gate, ins, key_cap=len(sc["keys"]), record_cap=4)  # exactly the rooms: enough
    capi._check(capi.lib().sk_check_device_errors())
    _same(sc, got, want, SLACK, record_cap, key_cap)


def _observed_descends(ps, pp, gs):
    o = gs[0]["observed"]
    o[0], o[1] = o[1], o[0]


def _read_off_descends(ps, pp, gs):
    pp[0]["read_off"][1] = pp[0]["read_off"][2] + 1


def _status_outside(ps, pp, gs):
    gs[0]["reads"]["status"][1] = 7


BAD = (("observed list", dict(mutate=_observed_descends)), ("read_off", dict(mutate=_read_off_descends)), ("gate status", dict(mutate=_status_outside)),
       ("record_cap is below", dict(record_cap=1)))


def test_bad_device_input_raises_the_flag_and_leaves_zeros(scenes):
    """an observed list that is not ascending, a read_off that is not monotone, a gate status outside the enum, a record capacity below the passing count: the
    _dev entry raises SK_DEVERR_REALIGN_PREAMBLE and leaves every output zero; the host entry refuses each with a message"""
    _needs_own_context()
    L = capi.lib()
    sc, gate, ins, want = next(x for x in scenes if x[0]["name"] == "cap_obs")
    assert want["totals"][0] == 1
    for text, kw in BAD:
        got, key_cap, record_cap = _dev(sc, gate, ins, **kw)
        assert L.sk_check_device_errors() != 0 and "sk_realign_preamble_dev" in capi.last_error() and L.sk_check_device_errors() == 0, text
        for name in ("records", "source", "consulted"):
            cap = key_cap if name == "consulted" else record_cap
            assert not got[name][:cap].view(np.uint8).any() and (got[name][cap:].view(np.uint8) == 0x5a).all(), (text, name)
        assert not any(got["totals"]) and all(not st[:2].any() and (st[2:] == 0x5a).all() for st in got["status"]), text
        ps, pp = P.packed(sc)
        gs = [dict(reads=g["reads"].copy(), observed_off=g["observed_off"].copy(), observed=g["observed"].copy(), observed_cap=g["observed_cap"]) for g in gate["samples"]]
        if "mutate" in kw:
            kw["mutate"](ps, pp, gs)
        with pytest.raises(capi.StrelkaAmdError, match=text):
            capi.realign_preamble(ps, dict(gate, samples=gs), pp, ins, sc["ref"], sc["ref_offset"], sc["max_indel_size"], record_cap=kw.get("record_cap"))
    got, key_cap, record_cap = _dev(sc, gate, ins, n_keys=len(sc["keys"]) + 9)  # more keys than key_cap
    assert L.sk_check_device_errors() != 0 and not any(got["totals"])
    got, key_cap, record_cap = _dev(sc, gate, ins)  # and the flag is gone: the same arrays, unharmed, give the result
    capi._check(L.sk_check_device_errors())
    _same(sc, got, want, SLACK, record_cap, key_cap)


def _job_results(job, first, n):
    return [repr(job.result(first + i)) for i in range(n)]


def _run(job):
    """-> None, or the message the run refuses with (both jobs then refuse alike)"""
    try:
        job.run()
        return None
    except capi.StrelkaAmdError as e:
        return str(e)


def test_prepared_job_equals_the_plain_job(scenes):
    """per scene and sample: a job fed by add_reads_prepared with the DEVICE's records (the reads the preamble declined go through plain add_reads in the same job)
    against a job fed by plain add_reads with all reads: every sk_read_result equal by repr, and
        the plain jobs' consulted marks == gate_consulted | preamble_consulted | the prepared jobs' marks
    over the samples of a scene (they share the table and the marks).  Reads the job refuses outright (a missing exemplar key, a spliced read) are handed to
    neither.  Scenes with an undecided key keep out of the marks' identity: the job's gate cannot ask what is not decided."""
    n_prepared = n_declined = n_searched = 0
    for sc, gate, ins, want in scenes:
        got = P.preamble(sc, False, gate, ins)
        nk = len(sc["keys"])
        plain_marks, prepared_marks = np.zeros(nk, np.uint8), np.zeros(nk, np.uint8)
        for s, sm in enumerate(sc["samples"]):
            indels, reads = P.job_inputs(sc, gate, ins, s)
            status = [int(x) for x in got["status"][s][:len(reads)]]
            gate_status = [int(x) for x in gate["samples"][s]["reads"]["status"][:len(reads)]]
            taken = [r for r in range(len(reads)) if status[r] not in (capi.RPRE_EDGE_KEY_MISSING, capi.RPRE_EXEMPLAR_KEY_MISSING) and gate_status[r] != capi.RGATE_SPLICED]
            ok = [r for r in taken if status[r] == capi.RPRE_OK]
            declined = [r for r in taken if status[r] != capi.RPRE_OK]
            if not taken:
                continue
            plain, prepared = P.new_job(sc, 2), P.new_job(sc, 2)
            plain.set_indels(indels)
            prepared.set_indels(indels)
            assert plain.add_reads([reads[r] for r in taken]) == 0
            src = [(int(x["sample"]), int(x["read"])) for x in got["source"][:got["totals"][0]]]
            recs = got["records"][[src.index((s, r)) for r in ok]] if ok else np.zeros(0, capi.REALIGN_PREPARED_READ_DTYPE)
            assert prepared.add_reads_prepared([reads[r] for r in ok], recs) == 0
            if declined:
                assert prepared.add_reads([reads[r] for r in declined]) == len(ok)
            refusal = _run(plain)
            assert _run(prepared) == refusal, (sc["name"], s, refusal)
            if refusal is None:
                a = dict(zip(taken, _job_results(plain, 0, len(taken))))
                b = dict(zip(ok + declined, _job_results(prepared, 0, len(taken))))
                for r in taken:
                    assert a[r] == b[r], (sc["name"], s, r, capi.RPRE_NAMES[status[r]])
                n_searched += sum("'n_cals': 0" not in a[r] for r in ok)
            n_prepared += len(ok)
            n_declined += len(declined)
            if nk:
                plain_marks |= plain.indels_consulted()
                prepared_marks |= prepared.indels_consulted()
        if nk and not any(c["undecided"] != CM.DECIDED for c in sc["cands"]):
            mine = gate["keys"]["gate_consulted"].astype(np.uint8) | got["consulted"][:nk] | prepared_marks
            assert (plain_marks == mine).all(), (sc["name"], plain_marks, mine)
    assert n_prepared > 500 and n_declined > 100 and n_searched > 100


def test_add_reads_prepared_refuses_and_then_runs(scenes):
    """enumeration != 2, an index outside the table, n_sm above 40, a quality of 71: each refused with a message, nothing added; the untouched records then run"""
    sc, gate, ins, want = next(x for x in scenes if x[0]["name"] == "usability")
    got = P.preamble(sc, False, gate, ins)
    indels, reads = P.job_inputs(sc, gate, ins, 0)
    recs = got["records"][:2].copy()

    def refused(text, enumeration=2, recs=recs, reads=reads):
        job = P.new_job(sc, enumeration)
        job.set_indels(indels)
        with pytest.raises(capi.StrelkaAmdError, match=text):
            job.add_reads_prepared(reads, recs)
        assert job.n_reads() == 0
    refused("enumeration == 2", enumeration=0)
    bad = recs.copy()
    bad[1]["order"][0] = len(indels)
    refused("read 1: prepared record: an order entry that is not in the status map", recs=bad)
    bad = recs.copy()
    bad[0]["n_status"] = 41
    refused("read 0: prepared record: a count above", recs=bad)
    refused("quality score 71", reads=[(r[0], [30] * (len(r[0]) - 1) + [71]) + tuple(r[2:]) for r in reads])
    job = P.new_job(sc, 2)
    job.set_indels(indels)
    assert job.add_reads_prepared(reads, recs) == 0
    job.run()
    assert all(job.result(i)["n_cals"] > 0 for i in range(2))


def test_preamble_behind_the_device_chain_on_one_stream(scenes):
    """per sample sk_read_intake_dev -> sk_region_haplotypes_dev -> sk_region_alleles_dev, then sk_indel_table_dev -> sk_read_depth_dev (per sample) ->
    sk_indel_candidates_dev -> sk_realign_gate_dev -> sk_realign_preamble_dev, all on one stream with no host copy in between and the key count left on the
    device: the recorded two-sample scene under the germline configuration, against the core on the host over the model's gate"""
    import torch
    _needs_own_context()
    from tests import indel_table_model as T
    from tests import test_region_haplotypes as RH
    L = capi.lib()
    psc, pgate, pins, want = next(x for x in scenes if x[0]["name"] == "two_samples_one_deletion@germline")
    assert want["totals"][0] > 0
    grec = next(r for r in GM.golden()["scenes"] if r["name"] == psc["name"])
    rec = GM.candidate_scene(grec)
    sc = CM.scene_document(rec)
    samples, regions = T.scene_samples(sc)
    gate_samples = psc["samples"]
    copt, sets = CM.config_options(CM.golden()["configs"]["germline"], rec)
    win_begin, n_pos = rec["win_begin"], rec["n_pos"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()
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
    depth_scratch_bytes = L.sk_read_depth_scratch_bytes(n_pos)
    d_sets = dev(K.rate_set_arrays(sets).view(np.uint8))
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep, structs, n_bases = [], [], 0
    for sm, gs in zip(samples, gate_samples):
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
                 iat=dev(np.array(sm["iat"] + [0], np.uint8)), depth1=torch.full((n_pos + 1,), -1, dtype=torch.int32, device="cuda"),
                 depth2=torch.full((n_pos + 1,), -1, dtype=torch.int32, device="cuda"), dscratch=torch.zeros(depth_scratch_bytes, dtype=torch.uint8, device="cuda"),
                 read_len=dev(np.array([r["read_len"] for r in gs["reads"]] + [0], np.int32)), realign_begin=dev(np.array([r["realign"][0] for r in gs["reads"]] + [0], np.int32)),
                 realign_end=dev(np.array([r["realign"][1] for r in gs["reads"]] + [0], np.int32)))
        i_scratch_bytes = L.sk_read_intake_scratch_bytes(n, n_segs, 0)
        x["iscratch"] = torch.zeros(max(i_scratch_bytes, 1), dtype=torch.uint8, device="cuda")
        capi._check(L.sk_read_intake_dev(p(d["ref"]), sc["ref_offset"], len(sc["ref"]), n, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]), C.byref(opt), 0, 0,
                                         p(x["reads"]), p(x["obs_off"]), p(x["obs"]), cap, p(x["sites"]), p(x["cand"]), p(x["iscratch"]), i_scratch_bytes, st))
        d["obs_off"], d["obs"] = x["obs_off"], x["obs"]
        RH._dev_launch(c, d, d_regions, d_n, st)
        capi._check(L.sk_region_alleles_dev(p(d["ref"]), sc["ref_offset"], len(sc["ref"]), p(d_regions), p(d_n), region_cap, p(d["recs"]), p(d["seq"]), d["seq_cap"],
                                            sc["max_indel_size"], max_hap_len, sc["prev_end_in"], p(x["arecs"]), p(x["alleles"]), allele_cap, p(x["ins"]), insert_cap,
                                            p(x["atotals"]), p(x["prev"]), p(x["ascratch"]), a_scratch_bytes, st))
        keep.append((d, x, n, n_segs, cap))
        q = lambda tensor: tensor.data_ptr()
        structs.append(capi.IndelTableSample(n, 0, q(t[0]), q(t[1]), q(x["obs_off"]), q(x["obs"]), cap, q(x["align_id"]), q(x["iat"]), q(d["recs"]), q(d["support"]),
                                             d["support_cap"], q(x["arecs"]), q(x["alleles"]), allele_cap, q(x["ins"]), insert_cap))
        n_bases += sum(len(r["code"]) for r in sm["reads"])
    n_samples = len(samples)
    arr = (capi.IndelTableSample * n_samples)(*structs)
    expand_cap, key_cap, id_cap, ins_cap = 4096, 512, 4096, n_bases + 1024
    n_reads = sum(k[2] for k in keep)
    room = lambda n, itemsize: torch.full(((n + SLACK) * itemsize,), 0x5a, dtype=torch.uint8, device="cuda")
    out = dict(keys=torch.zeros(key_cap * 56, dtype=torch.uint8, device="cuda"), data=torch.zeros(key_cap * n_samples * 64, dtype=torch.uint8, device="cuda"),
               ids=torch.zeros(id_cap, dtype=torch.int32, device="cuda"), ins=torch.zeros(ins_cap, dtype=torch.uint8, device="cuda"),
               totals=torch.full((4,), -1, dtype=torch.int64, device="cuda"), cand=torch.full((key_cap * 8,), 0x5a, dtype=torch.uint8, device="cuda"),
               rates=torch.full((key_cap * n_samples * 32,), 0x5a, dtype=torch.uint8, device="cuda"), ctotals=torch.full((2,), -1, dtype=torch.int64, device="cuda"),
               gkeys=room(key_cap, 48), glogs=room(key_cap * n_samples, 16), gtotals=torch.full((2 + capi.MAX_SAMPLES,), -1, dtype=torch.int64, device="cuda"),
               records=room(n_reads, 784), source=room(n_reads, 8), consulted=room(key_cap, 1), ptotals=torch.full((capi.RPRE_N_TOTALS,), -1, dtype=torch.int64, device="cuda"))
    scratch_bytes = L.sk_indel_table_scratch_bytes(n_samples, expand_cap, region_cap)
    scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    c_scratch_bytes = L.sk_indel_candidates_scratch_bytes()
    c_scratch = torch.zeros(c_scratch_bytes, dtype=torch.uint8, device="cuda")
    g_scratch_bytes = L.sk_realign_gate_scratch_bytes(n_samples, key_cap, id_cap)
    g_scratch = torch.full((g_scratch_bytes,), 0xa5, dtype=torch.uint8, device="cuda")
    p_scratch_bytes = capi.realign_preamble_scratch_bytes(n_samples, key_cap, n_reads)
    p_scratch = torch.full((p_scratch_bytes,), 0xa5, dtype=torch.uint8, device="cuda")
    d_ref = dev(np.frombuffer(sc["ref"].encode() + b"\0", np.uint8))
    _, pp = P.packed(psc)
    capi._check(L.sk_indel_table_dev(n_samples, C.addressof(arr), keep[0][0]["ref"].data_ptr(), sc["ref_offset"], len(sc["ref"]), d_regions.data_ptr(), d_n.data_ptr(), region_cap,
                                     sc["prev_end_in"], expand_cap, out["keys"].data_ptr(), key_cap, out["data"].data_ptr(), out["ids"].data_ptr(), id_cap, out["ins"].data_ptr(),
                                     ins_cap, out["totals"].data_ptr(), scratch.data_ptr(), scratch_bytes, st))
    cstructs, gin, gout, pre, statuses = [], [], [], [], []
    for (d, x, n, n_segs, cap), q in zip(keep, pp):
        t = d["t"]
        capi._check(L.sk_read_depth_dev(n, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), n_segs, t[5].data_ptr(), x["iat"].data_ptr(), win_begin, n_pos,
                                        x["depth1"].data_ptr(), x["depth2"].data_ptr(), x["dscratch"].data_ptr(), depth_scratch_bytes, st))
        cstructs.append(capi.IndelCandidateSample(n, 0, x["obs_off"].data_ptr(), x["obs"].data_ptr(), cap, x["depth1"].data_ptr(), x["depth2"].data_ptr()))
        gin.append(capi.RealignGateSample(n, 0, t[5].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), n_segs, x["read_len"].data_ptr(), x["align_id"].data_ptr(),
                                          x["realign_begin"].data_ptr(), x["realign_end"].data_ptr()))
        o = dict(reads=room(n, 12), observed_off=room(n + 1, 8), observed=room(id_cap, 4), code=dev(q["read_code"]), read_off=dev(q["read_off"]), fwd=dev(q["is_fwd_strand"]),
                 status=room(n, 1))
        x["gate"] = o
        statuses.append(o["status"])
        gout.append(capi.RealignGateSampleOut(o["reads"].data_ptr(), o["observed_off"].data_ptr(), o["observed"].data_ptr(), id_cap))
        pre.append(capi.RealignPreambleSample(o["code"].data_ptr(), o["read_off"].data_ptr(), q["code_cap"], o["fwd"].data_ptr(), o["status"].data_ptr()))
    carr = (capi.IndelCandidateSample * n_samples)(*cstructs)
    o = K.capi_options(copt)
    capi._check(L.sk_indel_candidates_dev(n_samples, C.addressof(carr), win_begin, n_pos, out["keys"].data_ptr(), out["data"].data_ptr(), out["totals"].data_ptr(), key_cap,
                                          d_sets.data_ptr(), C.addressof(o), out["cand"].data_ptr(), out["rates"].data_ptr(), out["ctotals"].data_ptr(), c_scratch.data_ptr(),
                                          c_scratch_bytes, st))
    garr_in, garr_out, parr = (capi.RealignGateSample * n_samples)(*gin), (capi.RealignGateSampleOut * n_samples)(*gout), (capi.RealignPreambleSample * n_samples)(*pre)
    capi._check(L.sk_realign_gate_dev(n_samples, C.addressof(garr_in), out["keys"].data_ptr(), out["data"].data_ptr(), out["ids"].data_ptr(), out["totals"].data_ptr(), key_cap, id_cap,
                                      out["cand"].data_ptr(), out["rates"].data_ptr(), sc["max_indel_size"], out["gkeys"].data_ptr(), out["glogs"].data_ptr(), C.addressof(garr_out),
                                      out["gtotals"].data_ptr(), g_scratch.data_ptr(), g_scratch_bytes, st))
    capi.realign_preamble_dev(n_samples, C.addressof(garr_in), C.addressof(garr_out), C.addressof(parr), out["gkeys"].data_ptr(), out["totals"].data_ptr(), key_cap,
                              out["ins"].data_ptr(), ins_cap, d_ref.data_ptr(), sc["ref_offset"], len(sc["ref"]), sc["max_indel_size"], out["records"].data_ptr(),
                              out["source"].data_ptr(), n_reads, out["consulted"].data_ptr(), out["ptotals"].data_ptr(), p_scratch.data_ptr(), p_scratch_bytes, st)
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    assert int(out["totals"].cpu().numpy()[0]) == len(psc["keys"])
    got = dict(records=out["records"].cpu().numpy().view(capi.REALIGN_PREPARED_READ_DTYPE), source=out["source"].cpu().numpy().view(capi.REALIGN_PREPARED_SOURCE_DTYPE),
               consulted=out["consulted"].cpu().numpy(), totals=out["ptotals"].cpu().numpy().tolist(), status=[s.cpu().numpy() for s in statuses])
    _same(psc, got, want, SLACK, n_reads, key_cap)
