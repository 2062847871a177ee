"""The realignment preamble's container-free core (csrc/preamble_core.h) against the job's own preamble (host/read_realign.cpp: enumerate_read ->
get_candidate_alignments -> to_core_read), on the host: sk_debug_realign_preamble_host runs the core over host arrays through the argument record the
kernels take, sk_debug_realign_job_prepared returns what the container-based statement makes of a read of a job.  No device is needed: the gate's
outputs come from the loop model (tests/realign_gate_model.py), and a job with enumeration == 2 leaves the search pending when a read is added.

The scenes are the 82 recorded gate scenes and the crafted windows of tests/realign_preamble_cases.py."""
import numpy as np
import pytest

from strelka_amd import capi
from tests import indel_candidates_model as CM
from tests import realign_gate_model as GM
from tests import realign_preamble_cases as P

NAMES = capi.RPRE_NAMES


@pytest.fixture(scope="module")
def runs():
    """every scene once: (scene, gate, insert pool, the model's gate result, the core's result on the host, the job's preamble per read, the job's marks over all
    reads, its marks over the passing reads)"""
    out = []
    for sc in P.all_scenes():
        gate, ins, want = P.model_gate(sc)
        core = P.preamble(sc, True, gate, ins, slack=2)
        job, marks_all, marks_pass = P.job_preamble(sc, gate, ins)
        out.append((sc, gate, ins, want, core, job, marks_all, marks_pass))
    return out


def _status_names(sc, core):
    return {(s, r): NAMES[int(x)] for s, sm in enumerate(sc["samples"]) for r, x in enumerate(core["status"][s][:len(sm["reads"])])}


def test_core_records_equal_the_jobs_byte_for_byte(runs):
    """every passing read of every scene: the core's record equals sk_debug_realign_job_prepared's in all 784 bytes, padding included; where the job declines
    (a capacity, a negative position) or refuses (a missing key) the core's status says so; records, source and totals are consistent and nothing is
    written behind the arrays"""
    n_records = n_declined = 0
    for sc, gate, ins, want, core, job, _, _ in runs:
        status = _status_names(sc, core)
        n_rec = core["totals"][0]
        assert (core["records"][len(core["records"]) - 2:].view(np.uint8) == 0x5a).all() and (core["source"][len(core["source"]) - 2:].view(np.uint8) == 0x5a).all()
        assert (core["consulted"][len(sc["keys"]):] == 0x5a).all() and all((st[len(sm["reads"]):] == 0x5a).all() for st, sm in zip(core["status"], sc["samples"]))
        assert not core["records"][n_rec:len(core["records"]) - 2].view(np.uint8).any(), sc["name"]  # the room past the records stays zero
        source = [(int(x["sample"]), int(x["read"])) for x in core["source"][:n_rec]]
        assert source == sorted(k for k, v in status.items() if v == "OK"), sc["name"]  # compacted in (sample, read) order
        assert core["totals"][1:] == [sum(v == n for v in status.values()) for n in NAMES], sc["name"]
        for (s, r), name in status.items():
            passed = want["samples"][s]["reads"][r]["status"] == GM.PASS
            kind, rec = job[(s, r)]
            assert (name == "NOT_PASSED") == (not passed), (sc["name"], s, r)
            if name == "OK":
                got = core["records"][source.index((s, r))]
                assert kind == "OK" and got.tobytes() == rec.tobytes(), (sc["name"], s, r, got, rec)
                n_records += 1
            elif name in ("EDGE_KEY_MISSING", "EXEMPLAR_KEY_MISSING"):
                assert kind == name, (sc["name"], s, r, kind, rec)
            else:  # the gate, a capacity, a negative position: the job has no record either (a spliced read is refused outright)
                assert kind in ("NONE", "SPLICED"), (sc["name"], s, r, name, kind)
                n_declined += passed
            if (s, r) in sc["expect"]:
                assert name == sc["expect"][(s, r)], (sc["name"], s, r, name)
    assert n_records > 500 and n_declined >= 4


def test_preamble_consulted_is_what_the_job_asks_beyond_its_gate(runs):
    """The identity: for a job (enumeration == 2, the search left pending) given the reads that pass the gate,
        sk_realign_job_indels_consulted == (the keys those reads' gates asked, rule G4 read by read) | preamble_consulted,
    and preamble_consulted is a subset of it.  The search's marks are not in it: nothing has searched yet.  Over all reads the job's marks are
    gate_consulted | preamble_consulted.  Scenes with an undecided key are left out: the job's gate cannot ask what is not decided."""
    n = 0
    for sc, gate, ins, want, core, job, marks_all, marks_pass in runs:
        if any(c["undecided"] != CM.DECIDED for c in sc["cands"]):
            continue
        nk = len(sc["keys"])
        asked_pass = np.zeros(nk, np.uint8)
        for so in want["samples"]:
            for rd, asked in zip(so["reads"], so["asked"]):
                if rd["status"] == GM.PASS:
                    asked_pass[asked] = 1
        mine = core["consulted"][:nk]
        assert set(np.unique(mine)) <= {0, 1}
        assert (marks_pass == (asked_pass | mine)).all(), (sc["name"], marks_pass, asked_pass, mine)
        assert (marks_all == (np.array([k["gate_consulted"] for k in want["keys"]], np.uint8) | mine)).all(), sc["name"]
        n += int(mine.sum())
    assert n > 100


def _record_of(sc_name, runs, s, r):
    for sc, gate, ins, want, core, job, _, _ in runs:
        if sc["name"] == sc_name:
            src = [(int(x["sample"]), int(x["read"])) for x in core["source"][:core["totals"][0]]]
            return sc, core, core["records"][src.index((s, r))]
    raise KeyError(sc_name)


def test_the_crafted_windows_reach_every_branch(runs):
    """the cases file itself, through the hooks alone: every SK_RPRE_* status a read can reach occurs, every scene but the declined ones yields a record, and
    every branch the rules name leaves its trace in a record.  SK_RPRE_EDGE_KEY_MISSING cannot occur: rule P1 matchifies both edges of a DNA read (the
    reference pins edges for RNA segments only), so no INSERT or DELETE stands outside the match segments when rule P2 looks, whether the table holds its
    key or not -- the two edge scenes show exactly that; the core keeps the status because the host keeps the Fail."""
    seen = set()
    crafted = {sc["name"] for sc in P.crafted()}
    for sc, gate, ins, want, core, job, _, _ in runs:
        if sc["name"] not in crafted:
            continue
        status = _status_names(sc, core)
        seen |= set(status.values())
        assert set(status) == set(sc["expect"]), sc["name"]
        for k, v in sc["expect"].items():  # every read that is not declined yields a record
            assert (job[k][0] == "OK") == (v == "OK"), (sc["name"], k)
    assert seen == set(NAMES) - {"NONE", "EDGE_KEY_MISSING"}, seen
    path = lambda rec: [(int(t), int(n)) for t, n in rec["alignment"]["path"][:int(rec["alignment"]["n_seg"])]]
    smap = lambda rec: {int(e["idx"]): (int(e["is_present"]), int(e["is_remove_only"]), int(e["in_original"])) for e in rec["status_map"][:int(rec["n_status"])]}
    # a soft-clipped read: the clips are match and the position moved; a hard-clipped one: the counts are kept and the path is without them
    sc, core, rec = _record_of("clips", runs, 0, 0)
    assert path(rec) == [(P.M, 40)] and int(rec["alignment"]["pos"]) == 50 and not int(rec["clipped"]) and int(rec["read_length"]) == 40
    sc, core, rec = _record_of("clips", runs, 0, 1)
    assert path(rec) == [(P.M, 40)] and int(rec["clipped"]) and (int(rec["hc_lead"]), int(rec["hc_trail"])) == (3, 2) and not int(rec["alignment"]["is_fwd_strand"])
    sc, core, rec = _record_of("clips", runs, 0, 2)
    assert path(rec) == [(P.M, 37)] and int(rec["alignment"]["pos"]) == 52 and int(rec["hc_lead"]) == 2 and (int(rec["sc_lead"]), int(rec["sc_trail"])) == (0, 0)
    # edge indels, their keys present and absent: the same records but for the table's indices, and no edge index either way
    for name in ("edge_indels_present", "edge_indels_absent"):
        for r, (pos, length) in enumerate(((57, 33), (60, 30), (58, 30))):
            sc, core, rec = _record_of(name, runs, 0, r)
            assert path(rec) == [(P.M, length)] and int(rec["alignment"]["pos"]) == pos and (int(rec["alignment"]["lead"]), int(rec["alignment"]["trail"])) == (-1, -1), (name, r)
    # a swap below the maximum: one present key with both lengths; above: the breakpoint pair
    sc, core, rec = _record_of("swap_below", runs, 0, 0)
    present = [k for k, v in smap(rec).items() if v[0]]
    assert [(sc["keys"][k]["del_len"], sc["keys"][k]["ins"]) for k in present] == [(3, "GT")] and smap(rec)[present[0]][2] == 1
    sc, core, rec = _record_of("swap_above", runs, 0, 0)
    assert sorted(sc["keys"][k]["type"] for k, v in smap(rec).items() if v[0]) == [CM.BP_LEFT, CM.BP_RIGHT]
    # remove-only, and it goes last in the order
    sc, core, rec = _record_of("remove_only", runs, 0, 0)
    ro = [k for k, v in smap(rec).items() if v[1]]
    assert len(ro) == 1 and sc["keys"][ro[0]]["pos"] == 47 and int(rec["order"][int(rec["n_order"]) - 1]) == ro[0] and ro[0] == min(smap(rec))
    # observed but no candidate: usable for the read that observed it only; neither: asked, and in nobody's map
    sc, core, rec = _record_of("usability", runs, 0, 0)
    k_obs, k_none = [i for i, k in enumerate(sc["keys"]) if k["pos"] == 60][0], [i for i, k in enumerate(sc["keys"]) if k["pos"] == 62][0]
    assert k_obs in smap(rec) and k_none not in smap(rec) and [int(x) for x in rec["observed"][:int(rec["n_observed"])]] == [k_obs]
    assert k_obs not in smap(_record_of("usability", runs, 0, 1)[2]) and core["consulted"][k_none] == 1 and core["consulted"][k_obs] == 1
    # the last base of the insert decides; a read past its codes finds the key whose insert ends in N
    sc, core, rec = _record_of("insert_last_base", runs, 0, 1)
    assert [sc["keys"][k]["ins"] for k, v in smap(rec).items() if v[0]] == ["ACT"]
    sc, core, rec = _record_of("past_codes", runs, 0, 0)
    assert [sc["keys"][k]["ins"] for k, v in smap(rec).items() if v[0]] == ["ACN"]
    # the recompute: the found mismatch key is a segment of its own, the other mismatch is not
    sc, core, rec = _record_of("mismatch_recompute", runs, 0, 0)
    assert path(rec) == [(P.M, 5), (P.X, 1), (P.M, 34)] and [sc["keys"][k]["type"] for k, v in smap(rec).items() if v[0]] == [CM.MISMATCH]
    assert path(_record_of("mismatch_recompute", runs, 0, 1)[2]) == [(P.M, 40)]
    # exactly at the capacities
    assert int(_record_of("cap_k", runs, 0, 1)[2]["n_status"]) == capi.RPRE_K and int(_record_of("cap_obs", runs, 0, 1)[2]["n_observed"]) == capi.RPRE_OBS
    assert int(_record_of("cap_p", runs, 0, 1)[2]["alignment"]["n_seg"]) == 47
    assert int(_record_of("negative_pos", runs, 0, 1)[2]["alignment"]["pos"]) == 0
    # two samples
    sc, core, rec = _record_of("two_samples", runs, 1, 1)
    assert int(rec["sample"]) == 1 and [sc["keys"][k]["pos"] for k, v in smap(rec).items() if v[0]] == [60]
    assert [(int(x["sample"]), int(x["read"])) for x in core["source"][:core["totals"][0]]] == [(0, 0), (1, 0), (1, 1), (1, 2)]


def _small():
    sc = next(s for s in P.crafted() if s["name"] == "usability")
    gate, ins, _ = P.model_gate(sc)
    return sc, gate, ins


def test_the_hook_refuses_what_the_host_entry_refuses():
    sc, gate, ins = _small()

    def refused(text, gate=gate, mutate=None, **kw):
        ps, pp = P.packed(sc)
        if mutate:
            mutate(ps, pp)
        with pytest.raises(capi.StrelkaAmdError, match=text):
            capi.realign_preamble(ps, gate, pp, ins, sc["ref"], sc["ref_offset"], sc["max_indel_size"], host=True, **kw)
    g = dict(gate, samples=[dict(gate["samples"][0], observed=gate["samples"][0]["observed"].copy())])
    g["samples"][0]["observed"][0] = 7
    refused("observed list", gate=g)
    g = dict(gate, samples=[dict(gate["samples"][0], reads=gate["samples"][0]["reads"].copy())])
    g["samples"][0]["reads"]["status"][1] = 9
    refused("gate status", gate=g)
    refused("read_off", mutate=lambda ps, pp: pp[0]["read_off"].__setitem__(1, 200))
    refused("record_cap is below", record_cap=1)
    refused("segment type", mutate=lambda ps, pp: ps[0]["path"].__setitem__((0, 0), 11))


def test_add_reads_prepared_refuses_without_a_device():
    """what sk_realign_job_add_reads_prepared refuses, each with a message, nothing added: enumeration != 2, an index outside the table, n_sm above 40, a
    quality of 71, and a table that was not given in key order"""
    sc, gate, ins = _small()
    core = P.preamble(sc, True, gate, ins)
    indels, reads = P.job_inputs(sc, gate, ins, 0)
    recs = core["records"][:2].copy()

    def refused(text, enumeration=2, recs=recs, reads=reads, indels=indels):
        job = P.new_job(sc, enumeration)
        job.set_indels(indels)
        with pytest.raises(capi.StrelkaAmdError, match=text):
            job.add_reads_prepared(reads, recs)
        assert job.n_reads() == 0
    refused("enumeration == 2", enumeration=0)
    bad = recs.copy()
    bad[1]["status_map"][0]["idx"] = len(indels)
    refused("read 1: prepared record: a status map index outside", recs=bad)
    bad = recs.copy()
    bad[0]["n_status"] = 41
    refused("read 0: prepared record: a count above", recs=bad)
    hot = [(r[0], [30] * (len(r[0]) - 1) + [71]) + tuple(r[2:]) for r in reads]
    refused("quality score 71", reads=hot)
    refused("key order", indels=indels[::-1])
    job = P.new_job(sc, 2)
    job.set_indels(indels)
    assert job.add_reads_prepared(reads, recs) == 0 and job.n_reads() == 2 and not job.indels_consulted().any()  # no gate, no preamble: no marks
