"""F5 (flatten_score_kernel) against the staged chain ($SK_A5_FUSED=0) and the host path (enumeration = 0) on jobs that reach every
path of its prologue: the haplotype pool filled from the job's code images (reference windows that leave the reference on the left
and on the right, window starts at every residue mod 16), reads at every byte offset mod 4 of the job's read codes (the kernel loads
them byte by byte, so no path depends on it; the offsets are counted for the word form the issue describes), reads with no insert
sequence, reads over a stretch of nine inserts, one of them of 70 bases (more inserts, and a longer one, than the prologue keeps in
registers: the loop form), job tables
that fit the per-read table copy (at most 32 entries) and larger ones (the per-round copy), reads of 30-152 bases (the 152-base form)
and of 153-256 (the 256-base form).  The three give equal results, equal sets of consulted indels and equal counts of reference reads
outside the job's reference; the same job run twice gives the same (the read queue and the consulted masks leave no state); and F5
scored the jobs itself: at least three quarters of the device jobs completed as one fixed sequence.

What a read's pool holds (its window, the table's inserts between the lowest and the highest one its alignments name) is decided on
the device and not reported by it, so three of the cases are counted by what brings them about, not by what the device did: the
window's residue by the read's input position, and the stretch of inserts (one counter: the nine inserts and the 70-base one go
together) by reads whose input alignment spans the stretch with a margin.  The windows that leave the reference are counted from the
device's own count of reference reads outside, the tables from their sizes."""
import numpy as np
import pytest

from strelka_amd import capi, synth
from tests import f5_util as U

_BASES = "ACGT"
_INS_REGS = 4      # inserts the prologue keeps in registers (F5_INS_REG)
_TAB = 32          # entries of the per-read table copy (F5_TAB)
_KINDS = ("plain", "left", "right", "no_insert", "dense", "big_table")


def _span(rd):
    return sum(ln for t, ln in rd["path"] if t in (synth.SEG["MATCH"], synth.SEG["DELETE"]))


def _scenarios(seed, read_len, window, n):
    rng = np.random.default_rng(seed)
    scs = synth.realign_scenarios(n, rng, reads_per=10, max_indels=7, min_indels=4, read_len=read_len, window=window,
                                  haplotyping_rate=0.2)
    for i, sc in enumerate(scs):
        kind = _KINDS[i % len(_KINDS)]
        sc["kind"] = kind
        off, ref = sc["ref_offset"], sc["ref_seq"]
        used = {(d["pos"], d["del_len"], d["ins_seq"]) for d in sc["indels"]}

        def add(p, del_len, seq, cand):
            if (p, del_len, seq) in used:
                return
            used.add((p, del_len, seq))
            sc["indels"].append(dict(pos=p, type=synth.INDEL["INDEL"], del_len=del_len, ins_seq=seq, is_candidate=int(cand)))
        if kind == "no_insert":
            sc["indels"] = [d for d in sc["indels"] if not d["ins_seq"]]
        elif kind == "dense":
            # a stretch of inserts: a candidate at either end, non-candidates (one of 70 bases) between them -- a read whose alignments
            # name both ends holds all of them in its pool
            p0 = off + len(ref) // 2 - 20
            sc["stretch"] = (p0, p0 + 40)
            for k in range(8):
                seq = "".join(_BASES[int(x)] for x in rng.integers(0, 4, int(rng.integers(1, 4))))
                add(p0 + 5 * k + (5 if k == 7 else 0), 0, seq, k in (0, 7))
            add(p0 + 18, 0, "".join(_BASES[int(x)] for x in rng.integers(0, 4, 70)), False)
        elif kind == "big_table":
            # more entries than the per-read table copy holds: deletions in an extension of the reference that no read reaches
            ext = "".join(_BASES[int(x)] for x in rng.integers(0, 4, 520))
            for k in range(36):
                add(off + len(ref) + 80 + 11 * k, 1 + k % 3, "", False)
            ref = ref + ext
        if kind == "left":
            cut = int(rng.integers(40, 56))
            ref, off = ref[cut:], off + cut
        elif kind == "right":
            ref = ref[:len(ref) - int(rng.integers(60, 76))]
        sc["ref_seq"], sc["ref_offset"] = ref, off
        for rd in sc["reads"]:
            code, qual = rd["code"].copy(), rd["qual"].copy()
            L = len(code)
            code[rng.random(L) < 0.02] = 0    # '='
            code[rng.random(L) < 0.02] = 15   # N
            qual[rng.random(L) < 0.03] = 0
            qual[rng.random(L) < 0.03] = 70
            rd["code"], rd["qual"] = code, qual
    return scs


@pytest.mark.gpu
@pytest.mark.parametrize("seed,read_len,window", [(96201, (30, 153), (200, 360)), (96202, (153, 257), (330, 430))])
def test_f5_prologue_equals_staged_and_host(seed, read_len, window, monkeypatch):
    capi.init(0)
    scs = _scenarios(seed, read_len, window, 24)
    n_jobs = n_f5_jobs = n_reads = 0
    seen = dict(left=0, right=0, no_insert=0, insert_stretch=0, small_table=0, big_table=0)
    byte_off, residues, lens = set(), set(), []
    for sc in scs:
        out = {chain: U.run_chain(sc, chain, setenv=monkeypatch.setenv) for chain in ("host", "staged", "f5")}
        out["again"] = U.run_chain(sc, "f5", setenv=monkeypatch.setenv)
        f5 = out["f5"]
        print(sc["kind"], "jobs", f5["jobs"], "outside", [out[c]["outside"] for c in out], "consulted", sum(f5["consulted"]),
              "of", len(sc["indels"]))
        for chain in ("staged", "f5", "again"):
            assert out[chain]["res"] == out["host"]["res"], (sc["kind"], chain)
            assert out[chain]["consulted"] == out["host"]["consulted"], (sc["kind"], chain)
            assert out[chain]["outside"] == out["host"]["outside"], (sc["kind"], chain)
        handled = 0
        if f5["counts"][1] > 0:
            assert f5["jobs"] in ((1, 0, 0), (0, 1, 1)), f5["jobs"]
            assert out["again"]["jobs"] == f5["jobs"]
            n_jobs += 1
            n_f5_jobs += f5["jobs"][0]
            handled = f5["jobs"][0]
        # the cases, over the jobs F5 scored itself
        at = 0
        off, ref_end = sc["ref_offset"], sc["ref_offset"] + len(sc["ref_seq"])
        n_ins_tab = sum(1 for d in sc["indels"] if d["ins_seq"])
        for rd, r in zip(sc["reads"], f5["idx"]):
            if r is None:
                continue
            n_reads += 1
            lens.append(len(rd["code"]))
            if not handled:
                at += len(rd["code"])
                continue
            byte_off.add(at % 4)
            at += len(rd["code"])
            residues.add((rd["pos"] - off) % 16)
            seen["no_insert"] += n_ins_tab == 0
            if sc["kind"] == "dense" and rd["pos"] <= sc["stretch"][0] - 5 and rd["pos"] + _span(rd) >= sc["stretch"][1] + 5:
                seen["insert_stretch"] += 1   # (nine inserts in the stretch, more than _INS_REGS, one of them of 70 bases)
        if handled:
            seen["left"] += sc["kind"] == "left" and f5["outside"] > 0
            seen["right"] += sc["kind"] == "right" and f5["outside"] > 0
            seen["small_table"] += len(sc["indels"]) <= _TAB
            seen["big_table"] += len(sc["indels"]) > _TAB
    print("jobs", n_jobs, "as one sequence", n_f5_jobs, "reads", n_reads, "cases", seen, "byte offsets", sorted(byte_off),
          "window residues", sorted(residues))
    assert n_jobs >= len(scs) - 2 and n_f5_jobs >= 0.75 * n_jobs and n_reads > 120
    assert all(v > 0 for v in seen.values()), seen
    assert byte_off == {0, 1, 2, 3} and residues == set(range(16))
    assert max(lens) < read_len[1] and sum(read_len[0] <= n for n in lens) > 100
