"""F5 (flatten_score_kernel) against the staged chain ($SK_A5_FUSED=0) and the host path (enumeration = 0) on reads that reach
every case of its phase B: '=' and N read bases, qualities 0 and 70, N in the reference window, soft clips, non-candidate indels
(penalties before an op), inserts of 1-9 bases (ops that start at every read position mod 8), reads of 30-152 bases (the 152-base
form) and of 153-256 (the 256-base form), and reads with more than 64 and more than 128 candidate alignments.  The three give equal
results, and F5 scored the jobs itself: nearly all completed as one fixed sequence (a job with a read outside F5's form -- a pool over
768 bytes, more than 8 indels or 16 path segments in a record -- is run again the staged way, and is counted apart)."""
import numpy as np
import pytest

from strelka_amd import capi, synth
from tests import f5_util as U

_BASES = "ACGT"


def _scenarios(seed, read_len, window, n):
    rng = np.random.default_rng(seed)
    scs = synth.realign_scenarios(n, rng, reads_per=10, max_indels=9, min_indels=5, read_len=read_len, window=window,
                                  haplotyping_rate=0.2)
    for sc in scs:
        off, ref = sc["ref_offset"], sc["ref_seq"]
        # inserts of every length 1-9 (beside the scenario's own), some of them not candidates: their penalties precede ops
        used = {(d["pos"], d["del_len"], d["ins_seq"]) for d in sc["indels"]}
        for ln in range(1, 10):
            p = off + int(rng.integers(20, len(ref) - 20))
            seq = "".join(_BASES[int(x)] for x in rng.integers(0, 4, ln))
            if (p, 0, seq) in used:
                continue
            used.add((p, 0, seq))
            sc["indels"].append(dict(pos=p, type=synth.INDEL["INDEL"], del_len=0, ins_seq=seq, is_candidate=int(rng.random() < 0.5)))
        # N in the reference window (not where an insert copies from: those copies are made already)
        ref = list(ref)
        for i in rng.choice(len(ref), 3, replace=False):
            ref[int(i)] = "N"
        sc["ref_seq"] = "".join(ref)
        for rd in sc["reads"]:
            code, qual = rd["code"].copy(), rd["qual"].copy()
            L = len(code)
            code[rng.random(L) < 0.03] = 0    # '='
            code[rng.random(L) < 0.02] = 15   # N
            qual[rng.random(L) < 0.05] = 0
            qual[rng.random(L) < 0.05] = 70
            rd["code"], rd["qual"] = code, qual
    return scs


@pytest.mark.gpu
@pytest.mark.parametrize("seed,read_len,window", [(95101, (30, 153), (200, 360)), (95102, (153, 257), (330, 430))])
def test_f5_equals_staged_and_host(seed, read_len, window, monkeypatch):
    capi.init(0)
    scs = _scenarios(seed, read_len, window, 24)
    n_cals, n_reads, n_jobs, n_f5_jobs, n_clip, lens = [], 0, 0, 0, 0, []
    for sc in scs:
        out = {chain: U.run_chain(sc, chain, setenv=monkeypatch.setenv) for chain in ("host", "staged", "f5")}
        res = {chain: out[chain]["res"] for chain in out}
        f5, idx = out["f5"], out["f5"]["idx"]
        n_cals += [x["n_cals"] for x in f5["got"] if x is not None]
        one_wait, redone, staged = f5["jobs"]
        if f5["counts"][1] > 0:
            # F5 took every read of the job (one fixed sequence, nothing left to the staged chain), or turned one down and the
            # job ran again the staged way
            assert (one_wait, redone, staged) in ((1, 0, 0), (0, 1, 1)), (one_wait, redone, staged)
            n_jobs += 1
            n_f5_jobs += one_wait
        assert res["f5"] == res["host"]
        assert res["staged"] == res["host"]
        for rd, r in zip(sc["reads"], idx):
            if r is None:
                continue
            n_reads += 1
            lens.append(len(rd["code"]))
            n_clip += any(t == synth.SEG["SOFT_CLIP"] for t, _ in rd["path"])
    assert n_jobs >= len(scs) - 2 and n_f5_jobs >= 0.75 * n_jobs and n_reads > 120 and n_clip > 10
    assert max(lens) < read_len[1] and sum(read_len[0] <= n for n in lens) > 100
    assert max(n_cals) > 128 and sum(c > 64 for c in n_cals) > 5
