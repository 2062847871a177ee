"""What the realignment gate is for (sk_realign_gate; csrc/realign_gate.hip): its outputs are the arrays a realignment job is made of.

From the unit's outputs capi.realign_job_inputs builds sk_indel_info[] and sk_read_input[]; a second set is built the adapter's way from the
model's records (every key asked for its candidacy, the four id sets of every key inverted through a dict).  Both go through
sk_realign_job_add_reads / _run and every sk_read_result must be equal.  In addition a read the gate does not pass has no candidate
alignment in the job, and the job's consulted marks over ALL reads equal gate_consulted OR its marks over the passing reads alone: the
identity that lets a caller leave the failing reads at home.  No breakpoint keys in these scenes."""
import numpy as np
import pytest

from strelka_amd import capi
from tests import indel_candidates_model as CM
from tests import indel_table_model as T
from tests import realign_gate_cases as G
from tests import realign_gate_model as GM

pytestmark = pytest.mark.gpu

SCENES = ("gate_zone_edges", "gate_mismatch_edges", "gate_noise_and_support", "gate_clamped_at_0", "tiers_and_noise@germline", "two_samples_one_deletion@germline",
          "report_info@somatic", "report_info@germline")


def _adapter_inputs(keys, cands, doc, samples, sample):
    """the adapter's way, from the model's records: the map walked key by key, the id sets of every entry inverted through a dict"""
    indels = []
    for k, c in zip(keys, cands):
        logs = GM.log_rates(c["rates"][sample])
        indels.append(dict(pos=k["pos"], type=k["type"], del_len=k["del_len"], ins_seq=k["ins"], is_candidate=c["is_candidate"], r2i=CM.bits_double(logs[0]), i2r=CM.bits_double(logs[1]),
                           arid=k["active_region_id"], hap=[int(d["haplotype_id"]) for d in k["samples"]], bypass=[int(d["is_haplotyping_bypassed"] != 0) for d in k["samples"]]))
    by_id = {}
    for i, k in enumerate(keys):
        for ids in k["samples"][sample]["ids"]:
            for a in ids:
                by_id.setdefault(a, set()).add(i)
    reads = []
    for src, rd in zip(doc["samples"][sample]["reads"], samples[sample]["reads"]):
        reads.append((T.M.encode(src["seq"]), [30] * len(src["seq"]), rd["pos"], rd["path"], bool(src["is_fwd"]), _map_level(src["iat"]), sample, tuple(rd["realign"]),
                      sorted(by_id.get(src["id"], ()))))
    return indels, reads


def _map_level(iat):
    return (capi.MAPLEVEL["TIER1"], capi.MAPLEVEL["TIER2"], capi.MAPLEVEL["SUB"])[iat]


def _run_job(doc, n_samples, is_haplotyping_enabled, indels, reads, only=None):
    """-> ([repr of every read's result], the job's consulted marks); only: the indices of the reads to hand over"""
    job = capi.RealignJob(capi.realign_options(is_haplotyping_enabled=is_haplotyping_enabled, sample_count=n_samples, max_indel_size=doc["max_indel_size"]))
    job.set_reference(doc["ref"], doc["ref_offset"])
    job.set_indels(indels)
    chosen = [r for i, r in enumerate(reads) if only is None or i in only]
    if not chosen:
        return [], [0] * len(indels)
    first = job.add_reads(chosen)
    job.run()
    return [job.result(first + i) for i in range(len(chosen))], job.indels_consulted().tolist()


@pytest.mark.parametrize("name", SCENES)
def test_the_gates_outputs_make_the_job_the_adapter_makes(name):
    capi.init(0)
    rec = next(r for r in GM.golden()["scenes"] if r["name"] == name)
    csc = GM.candidate_scene(rec)
    doc = CM.scene_document(csc)
    keys, cands, samples, want = GM.run_recorded(rec)
    assert not any(k["type"] in (CM.BP_LEFT, CM.BP_RIGHT) for k in keys)
    ka, da, ids, ins = G.table_arrays(keys)
    ca, ra = G.cand_arrays(cands)
    gate = capi.realign_gate(G.packed_samples(samples), ka, da, ids, ca, ra, doc["max_indel_size"])
    hap = CM.golden()["configs"][csc["config"]]["is_haplotyping_enabled"]
    n_samples = len(samples)
    n_passing = n_failing = n_searched = 0
    all_marks, all_pass_marks = [0] * len(keys), [0] * len(keys)
    for s in range(n_samples):
        src = doc["samples"][s]["reads"]
        job_reads = [dict(code=T.M.encode(r["seq"]), qual=[30] * len(r["seq"]), pos=r["pos"], path=[tuple(t) for t in r["path"]], fwd=bool(r["is_fwd"]), map_level=_map_level(r["iat"]),
                          realign=samples[s]["reads"][i]["realign"]) for i, r in enumerate(src)]
        indels, reads = capi.realign_job_inputs(gate, s, job_reads, ins)
        a_indels, a_reads = _adapter_inputs(keys, cands, doc, samples, s)
        got, got_marks = _run_job(doc, n_samples, hap, indels, reads)
        exp, exp_marks = _run_job(doc, n_samples, hap, a_indels, a_reads)
        assert len(got) == len(exp) == len(src)
        for r, (g, e) in enumerate(zip(got, exp)):
            assert repr(g) == repr(e), (s, r)
        assert got_marks == exp_marks
        status = [int(x) for x in gate["samples"][s]["reads"]["status"]]
        passing = {r for r, st in enumerate(status) if st == capi.RGATE_PASS}
        assert all(st != capi.RGATE_UNDECIDED for st in status)
        for r, g in enumerate(got):  # a read the gate does not pass has no candidate alignment in the job
            assert r in passing or g["n_cals"] == 0, (s, r, status[r], g["n_cals"])
            n_searched += g["n_cals"] > 0
        _, pass_marks = _run_job(doc, n_samples, hap, indels, reads, only=passing)
        all_marks = [int(a or b) for a, b in zip(all_marks, got_marks)]
        all_pass_marks = [int(a or b) for a, b in zip(all_pass_marks, pass_marks)]
        mine = GM.consulted(len(keys), want["samples"][s]["asked"])  # this sample's share of gate_consulted: what its reads' gates asked
        assert got_marks == [int(a or b) for a, b in zip(mine, pass_marks)], (s, got_marks, mine, pass_marks)
        n_passing += len(passing)
        n_failing += len(src) - len(passing)
    # the jobs' marks over ALL reads == gate_consulted OR their marks over the passing reads only (the samples share the table and the marks)
    consulted = [int(x) for x in gate["keys"]["gate_consulted"]]
    assert all_marks == [int(a or b) for a, b in zip(consulted, all_pass_marks)], (all_marks, consulted, all_pass_marks)
    assert (n_passing > 0 and n_searched > 0) or name.endswith("@germline")
    if name in ("gate_zone_edges", "gate_overmax"):
        assert n_failing > 0
