"""Inputs of the realignment-preamble tests (sk_realign_preamble; csrc/realign_preamble.hip, csrc/preamble_core.h), shared by the host tests
(tests/test_realign_preamble_host.py) and the device tests (tests/test_realign_preamble.py): crafted windows, one per line of the rules P1-P5,
the 82 recorded gate scenes in the same form, and their conversion to the arrays of the entry points and to the inputs of a realignment job.
The gate's outputs come from the loop model (tests/realign_gate_model.py), so nothing here needs a device.

A scene: dict(name, ref, ref_offset, max_indel_size, hap, keys, cands, samples [dict(reads [dict(pos, path, read_len, realign, seq, fwd, n_code)],
align_id)], expect {(sample, read): RPRE name}); n_code: how many of the read's codes the preamble is given (the rest read 'N')."""
import functools

import numpy as np

from strelka_amd import capi
from tests import indel_candidates_model as CM
from tests import realign_gate_cases as G
from tests import realign_gate_model as GM

M, I, D, S, H = G.M, G.I, G.D, G.S, G.H
X = CM.SEG_SEQ_MISMATCH
CODE = {"=": 0, "A": 1, "C": 2, "G": 4, "T": 8}
CODE_CHAR = ["=ACNGNNNTNNNNNNN"[c] for c in range(16)]  # bam_seq::get_char
REF = ("GATTACAGGCTTACGATCCGATGCAATCGGTACCTAGGCATTGACCGTAAGCTTGACCATGGTCAAGCTAGGATCCTTAGCAGTCAAGGTCCATGACGTTAGCCATAGGACTTGCAATCGTAGGCTAACGTTCAGGACTTAGCCGATAC"
       "GGTTCAATGCGTACCGGATTACGCAATTGGCCTAGATCGGATACCTTGAAC")
assert len(REF) == 200


def encode(seq):
    return np.array([CODE.get(c, 15) for c in seq], np.uint8)


def _other(base):
    return "ACGT"[("ACGT".index(base) + 1) % 4]


def read(pos, path, ins="", realign=G.WIDE, fwd=True, mismatches=(), n_code=None):
    """a read whose bases are the reference's along its path; ins: the bases of its INSERT segments, one after the other; soft-clipped bases are T;
    mismatches: offsets in the read whose base is changed to another one"""
    seq, ref_at, ins_at = "", pos, 0
    for t, n in path:
        if t in (M, CM.SEG_SEQ_MATCH, X):
            seq += REF[ref_at:ref_at + n]
            ref_at += n
        elif t == I:
            seq += ins[ins_at:ins_at + n]
            ins_at += n
        elif t == S:
            seq += "T" * n
        elif t in (D, CM.SEG_SKIP):
            ref_at += n
    seq = list(seq)
    for at in mismatches:
        seq[at] = _other(seq[at])
    seq = "".join(seq)
    r = G.read(pos, path, realign)
    assert r["read_len"] == len(seq), (r["read_len"], len(seq))
    return dict(r, seq=seq, fwd=fwd, n_code=len(seq) if n_code is None else n_code)


def scene(name, keys, cands, samples, expect, max_indel_size=49, hap=0):
    order = sorted(range(len(keys)), key=lambda i: (keys[i]["pos"], keys[i]["type"], len(keys[i]["ins"]), keys[i]["del_len"], keys[i]["ins"].encode("latin-1")))
    return dict(name=name, ref=REF, ref_offset=0, max_indel_size=max_indel_size, hap=hap, keys=[keys[i] for i in order], cands=[cands[i] for i in order],
                samples=[dict(reads=reads, align_id=None) for reads in samples], expect=dict(expect))


def _seen(*reads):
    """id sets of a one-sample key observed by these reads (tier 1)"""
    return [[list(reads), [], [], []]]


@functools.lru_cache(maxsize=None)
def crafted():
    """the crafted windows, one per line the rules name; every read passes the gate through a candidate deletion its zone holds"""
    out = []
    anchor = lambda pos=70: (G.key(pos, del_len=2), G.cand(1))
    # P1: a soft-clipped read (the clips become match, the position moves left), a hard-clipped one (clip_clipper keeps the counts), both; one on the reverse strand
    k, c = anchor()
    out.append(scene("clips", [k], [c], [[read(55, [(S, 5), (M, 35)]), read(50, [(H, 3), (M, 40), (H, 2)], fwd=False), read(56, [(H, 2), (S, 4), (M, 30), (S, 3)])]],
                     {(0, 0): "OK", (0, 1): "OK", (0, 2): "OK"}))
    # P1/P2: a leading-edge insertion and a trailing-edge deletion, their keys in the table and not: both edges are matchified before P2 looks, so the
    # table is never asked for them
    for name, extra in (("edge_indels_present", [(G.key(60, ins="TGA"), G.cand(1)), (G.key(90, del_len=4), G.cand(1))]), ("edge_indels_absent", [])):
        k, c = anchor()
        out.append(scene(name, [k] + [e[0] for e in extra], [c] + [e[1] for e in extra],
                         [[read(60, [(I, 3), (M, 30)], ins="TGA"), read(60, [(M, 30), (D, 4)]), read(58, [(H, 1), (D, 2), (I, 2), (M, 25), (I, 1), (S, 2)], ins="ACG")]],
                         {(0, 0): "OK", (0, 1): "OK", (0, 2): "OK"}))
    # P4: a swap segment below max_indel_size (one key with both lengths) ...
    k, c = anchor()
    out.append(scene("swap_below", [k, G.key(65, del_len=3, ins="GT")], [c, G.cand(1)], [[read(50, [(M, 15), (I, 2), (D, 3), (M, 20)], ins="GT"), read(50, [(M, 40)])]],
                     {(0, 0): "OK", (0, 1): "OK"}))
    # ... and above it (the breakpoint pair): no single segment is over the maximum, which the gate would decline, but their sum is
    k, c = anchor()
    out.append(scene("swap_above", [k, G.key(65, CM.BP_LEFT, flags=CM.DO_NOT_GENOTYPE), G.key(68, CM.BP_RIGHT, flags=CM.DO_NOT_GENOTYPE)], [c, G.cand(1), G.cand(1)],
                     [[read(50, [(M, 15), (I, 6), (D, 3), (I, 6), (M, 20)], ins="GTGTGTACACAC")]], {(0, 0): "OK"}, max_indel_size=10))
    # P3: a key whose right end touches the range's begin: adjacent, not intersecting -> remove-only
    k, c = anchor()
    out.append(scene("remove_only", [k, G.key(47, del_len=3)], [c, G.cand(1)], [[read(50, [(M, 40)])]], {(0, 0): "OK"}))
    # P3: an observed key that is no candidate (usable), and a key that is neither (asked, not usable)
    k, c = anchor()
    out.append(scene("usability", [k, G.key(60, del_len=1, ids=_seen(0)), G.key(62, ins="A")], [c, G.cand(0), G.cand(0)], [[read(50, [(M, 40)]), read(52, [(M, 40)])]],
                     {(0, 0): "OK", (0, 1): "OK"}))
    # P4: the table's insert differs from the read's bases in the last base
    k, c = anchor()
    out.append(scene("insert_last_base", [k, G.key(65, ins="ACT")], [c, G.cand(1)],
                     [[read(50, [(M, 15), (I, 3), (M, 20)], ins="ACG"), read(50, [(M, 15), (I, 3), (M, 20)], ins="ACT")]], {(0, 0): "EXEMPLAR_KEY_MISSING", (0, 1): "OK"}))
    # P2/P4: a read running past its codes: the insert's last base and the base after it read 'N'
    k, c = anchor()
    out.append(scene("past_codes", [k, G.key(84, ins="ACN")], [c, G.cand(1)], [[read(50, [(M, 34), (I, 3), (M, 1)], ins="ACG", n_code=36)]], {(0, 0): "OK"}))
    # P4: a table with mismatch keys: the read has one of them (the recompute) and a mismatch the table does not hold (skipped)
    k, c = anchor()
    r = read(50, [(M, 40)], mismatches=(5, 12))
    out.append(scene("mismatch_recompute", [k, G.key(55, CM.MISMATCH, 1, r["seq"][5])], [c, G.cand(1)], [[r, read(50, [(M, 40)])]], {(0, 0): "OK", (0, 1): "OK"}))
    # the status map's capacity: 41 usable keys in one read's range, and exactly 40 in another's
    keys = [G.key(52 + 2 * i, del_len=1) for i in range(41)]
    out.append(scene("cap_k", keys, [G.cand(1)] * 41, [[read(50, [(M, 100)]), read(55, [(M, 95)])]], {(0, 0): "CAP_K", (0, 1): "OK"}))
    # the observed list's capacity: 65 entries, and exactly 64
    keys = [G.key(5 + 2 * i, del_len=1, ids=_seen(0, 1) if i < 64 else _seen(0)) for i in range(65)] + [G.key(160, del_len=2)]
    out.append(scene("cap_obs", keys, [G.cand(0)] * 65 + [G.cand(1)], [[read(150, [(M, 30)]), read(151, [(M, 30)])]], {(0, 0): "CAP_OBS", (0, 1): "OK"}))
    # the path's capacity: 51 segments whose 25 deletions the table holds
    keys = [G.key(51 + 2 * i, del_len=1) for i in range(25)]
    out.append(scene("cap_p", keys, [G.cand(1)] * 25, [[read(50, [(M, 1), (D, 1)] * 25 + [(M, 1)]), read(50, [(M, 1), (D, 1)] * 23 + [(M, 5)])]], {(0, 0): "CAP_P", (0, 1): "OK"}))
    # P1: a normalised position below 0
    out.append(scene("negative_pos", [G.key(10, del_len=2)], [G.cand(1)], [[read(2, [(S, 5), (M, 30)]), read(5, [(S, 5), (M, 30)])]], {(0, 0): "NEGATIVE_POS", (0, 1): "OK"}))
    # two samples: a key one sample observed, reads of both, one that leaves at the gate
    keys = [G.key(70, del_len=2, n_samples=2), G.key(60, del_len=1, ids=[[[], [], [], []], [[1], [], [], []]], n_samples=2)]
    out.append(scene("two_samples", keys, [G.cand(1, n_samples=2), G.cand(0, n_samples=2)],
                     [[read(50, [(M, 40)]), read(120, [(M, 40)])], [read(52, [(M, 30)], fwd=False), read(50, [(M, 10), (D, 1), (M, 29)]), read(54, [(S, 2), (M, 30)])]],
                     {(0, 0): "OK", (0, 1): "NOT_PASSED", (1, 0): "OK", (1, 1): "OK", (1, 2): "OK"}))
    return out


@functools.lru_cache(maxsize=None)
def recorded():
    """the recorded gate scenes (tests/golden/realign_gate) in the same form; expect is empty: the job's own preamble says what to expect"""
    out = []
    for rec in GM.golden()["scenes"]:
        csc = GM.candidate_scene(rec)
        doc = CM.scene_document(csc)
        keys, cands, samples, _ = GM.run_recorded(rec)
        reads = [[dict(rd, seq=src["seq"], fwd=bool(src["is_fwd"]), n_code=len(src["seq"])) for rd, src in zip(sm["reads"], dsm["reads"])] for sm, dsm in zip(samples, doc["samples"])]
        out.append(dict(name=rec["name"], ref=doc["ref"], ref_offset=doc["ref_offset"], max_indel_size=doc["max_indel_size"], hap=CM.golden()["configs"][csc["config"]]["is_haplotyping_enabled"],
                        keys=keys, cands=cands, samples=[dict(reads=r, align_id=sm["align_id"]) for r, sm in zip(reads, samples)], expect={}))
    return out


def all_scenes():
    return crafted() + recorded()


# ---- to the arrays of the entry points
def model_gate(sc):
    """the gate's outputs as capi.realign_gate returns them, from the loop model -> (gate, insert_pool, the model's result)"""
    want = GM.realign_gate(sc["keys"], sc["cands"], sc["samples"], sc["max_indel_size"])
    ka, _, _, ins = G.table_arrays(sc["keys"])
    n_samples = len(sc["samples"])
    keys = np.zeros(len(sc["keys"]), capi.REALIGN_GATE_KEY_DTYPE)
    logs = np.zeros(len(sc["keys"]) * n_samples, capi.REALIGN_GATE_LOG_RATES_DTYPE)
    for k, w in enumerate(want["keys"]):
        o = keys[k]
        o["pos"], o["type"], o["del_len"], o["ins_len"], o["ins_off"], o["active_region_id"] = w["pos"], w["type"], w["del_len"], len(w["ins"]), int(ka[k]["ins_off"]), w["active_region_id"]
        o["is_candidate"], o["undecided"], o["gate_consulted"] = w["is_candidate"], w["undecided"], w["gate_consulted"]
        o["haplotype_id"], o["is_haplotyping_bypassed"] = w["haplotype_id"], w["is_haplotyping_bypassed"]
        logs[k * n_samples:(k + 1) * n_samples] = np.array([b for row in w["logs"] for b in row], np.uint64).view(capi.REALIGN_GATE_LOG_RATES_DTYPE)
    samples = []
    for so in want["samples"]:
        reads = np.zeros(len(so["reads"]) + 1, capi.REALIGN_GATE_READ_DTYPE)
        for r, g in enumerate(so["reads"]):
            reads[r] = (g["zone"][0], g["zone"][1], g["status"], g["asked_undecided"], 0)
        off = np.cumsum([0] + [len(o) for o in so["observed"]]).astype(np.int64)
        flat = np.array([k for o in so["observed"] for k in o] + [0], np.int32)
        samples.append(dict(reads=reads, observed_off=off, observed=flat, observed_cap=int(off[-1])))
    return dict(keys=keys, logs=logs, samples=samples, totals=want["totals"]), ins, want


def packed(sc):
    """-> (pack_gate_sample's dicts, pack_preamble_sample's dicts)"""
    return ([capi.pack_gate_sample(sm["reads"], None) for sm in sc["samples"]],
            [capi.pack_preamble_sample([encode(r["seq"])[:r["n_code"]] for r in sm["reads"]], [r["fwd"] for r in sm["reads"]]) for sm in sc["samples"]])


def preamble(sc, host, gate=None, ins=None, **kw):
    """the scene through sk_realign_preamble (host=False) or sk_debug_realign_preamble_host (host=True) -> capi.realign_preamble's result"""
    if gate is None:
        gate, ins, _ = model_gate(sc)
    ps, pp = packed(sc)
    return capi.realign_preamble(ps, gate, pp, ins, sc["ref"], sc["ref_offset"], sc["max_indel_size"], host=host, **kw)


# ---- to a realignment job
def job_inputs(sc, gate, ins, sample):
    """-> (indels as RealignJob.set_indels takes them: the gate's keys in table order, reads as add_reads takes them; codes past n_code are N)"""
    src = []
    for r in sc["samples"][sample]["reads"]:
        code = encode(r["seq"])
        code[r["n_code"]:] = 15
        src.append(dict(code=code, qual=[30] * len(code), pos=r["pos"], path=r["path"], fwd=r["fwd"], realign=r["realign"]))
    return capi.realign_job_inputs(gate, sample, src, ins)


def new_job(sc, enumeration):
    job = capi.RealignJob(capi.realign_options(is_haplotyping_enabled=sc["hap"], sample_count=len(sc["samples"]), max_indel_size=sc["max_indel_size"], enumeration=enumeration))
    job.set_reference(sc["ref"], sc["ref_offset"])
    return job


def job_preamble(sc, gate, ins):
    """what the job's own preamble makes of every read, through sk_realign_job_add_read and sk_debug_realign_job_prepared alone ->
    ({(sample, read): ("OK", record) | ("NONE", None) | ("EDGE_KEY_MISSING" | "EXEMPLAR_KEY_MISSING" | "SPLICED", message)}, the jobs' consulted marks over
    all reads, their marks over the reads that pass the gate).  enumeration == 2: adding a read runs the gate and the preamble and leaves the search
    pending, so the marks are the gate's and the preamble's and no device is needed."""
    out = {}
    n_keys = len(sc["keys"])
    marks_all, marks_pass = np.zeros(n_keys, np.uint8), np.zeros(n_keys, np.uint8)
    for s in range(len(sc["samples"])):
        indels, reads = job_inputs(sc, gate, ins, s)
        job, job_pass = new_job(sc, 2), new_job(sc, 2)
        job.set_indels(indels)
        job_pass.set_indels(indels)
        for r, rd in enumerate(reads):
            passed = int(gate["samples"][s]["reads"]["status"][r]) == capi.RGATE_PASS
            try:
                i = job.add_read(*rd)
            except capi.StrelkaAmdError as e:
                msg = str(e)
                out[(s, r)] = ("EDGE_KEY_MISSING" if "edge indel" in msg else "EXEMPLAR_KEY_MISSING" if "Exemplar" in msg else "SPLICED" if "spliced" in msg else "?", msg)
                assert out[(s, r)][0] != "?", msg
            else:
                rec = job.debug_prepared(i)
                out[(s, r)] = ("NONE", None) if rec is None else ("OK", rec)
            if passed:
                try:
                    job_pass.add_read(*rd)
                except capi.StrelkaAmdError:
                    pass
        if n_keys:
            marks_all |= job.indels_consulted()
            marks_pass |= job_pass.indels_consulted()
    return out, marks_all, marks_pass
