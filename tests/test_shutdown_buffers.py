"""sk_shutdown leaves nothing of the library's on the device: every module's grown buffers are dropped (sk_debug_grown_bytes reports 0 and
0), what pointed into them is forgotten (a generation kept from before the shutdown is refused), and the same calls after another sk_init
give the same bytes.  The inputs are the smallest that grow every module's buffers: the context arena (read intake, region haplotypes and
alleles, gVCF runs, the deflate's input and output), the deflate's slots, tokens and slot lengths, and the enumeration job's buffers.

The region case is the first recorded scene of tests/region_haplotype_cases.py with its diploid regions; each of the first three golden
realignment scenarios is a job of its own (a job has one reference).  A change of device needs two GPUs and is not tested."""
import ctypes as C
import gc
import os
import pickle

import numpy as np
import pytest

from strelka_amd import capi
from tests import intake_cases, region_haplotype_cases
from tests import test_read_realign as T


def _fetch_score(generation):
    """-> sk_enum_device_fetch_scores' return value for the first score of run `generation`"""
    L = capi.lib()
    L.sk_enum_device_fetch_scores.argtypes = [C.c_uint64, C.c_int32, C.c_int32, C.c_void_p]
    score = C.c_double(0.0)
    return int(L.sk_enum_device_fetch_scores(generation, 0, 1, C.byref(score)))


def _run_everything(gold):
    """-> ({name: bytes} of every output, the last job's generation); the jobs' per-read results are checked against the golden expectation here"""
    out = {}
    c = intake_cases.crafted()[0]
    res = capi.read_intake(c["ref"], c["ref_offset"], c["reads"], c["low"], c["win_begin"], c["n_pos"])
    for k in ("reads", "obs_off", "obs", "sites", "is_candidate"):
        out["intake." + k] = res[k].tobytes()

    sc = region_haplotype_cases.golden()[0]
    regions = [(g["begin"], g["end"]) for g in sc["regions"] if g["ploidy"] == 2]
    haps = capi.region_haplotypes(sc["ref"], sc["ref_offset"], sc["reads"], sc["low"], sc["fwd"], regions, sc["buf_begin"], sc["buf_end"], 2, raw=True)
    for k in ("recs", "seq_pool", "support_pool", "query_off", "totals"):
        out["haplotypes." + k] = haps[k].tobytes()
    alleles = capi.region_alleles(sc["ref"], sc["ref_offset"], regions, haps, sc["max_indel_size"], 1024, -1, raw=True)
    for k in ("recs", "alleles", "insert_pool", "totals"):
        out["alleles." + k] = alleles[k].tobytes()
    out["alleles.prev_end_out"] = alleles["prev_end_out"]

    rng = np.random.default_rng(20260)
    n = 100
    used = rng.integers(20, 60, n).astype(np.uint32)
    sm = np.zeros(n, capi.GVCF_SITE_SUMMARY_DTYPE)
    sm["flags"] = rng.random(n) >= 0.05
    sm["gqx"] = np.minimum(99, 2 * used).astype(np.int32)
    sm["ref_fwd"] = used // 2
    sm["ref_rev"] = used - used // 2
    out["gvcf.runs"] = capi.gvcf_plain_runs(sm, used, used + 1, used + 2, capi.gvcf_block_options()).tobytes()

    data = rng.integers(0, 4, 70000).astype(np.uint8)  # (two blocks; four symbols, so that the dynamic codes have something to do)
    out["deflate"] = capi.bgzf_deflate(data, level=2)

    for si, (s, exp) in enumerate(zip(gold["scenarios"][:3], gold["expect"][:3])):
        job = capi.RealignJob(capi.realign_options(is_haplotyping_enabled=s["is_haplotyping_enabled"], min_read_bp_flank=s["min_read_bp_flank"], enumeration=2))
        job.set_reference(s["ref_seq"], s["ref_offset"])
        job.set_indels(s["indels"])
        idx = T._add_reads(job, s)
        job.run()
        for ri, (i, want) in enumerate(zip(idx, exp)):
            T._check_read(s, None if i is None else job.result(i), want, "scenario %d read %d" % (si, ri))
        out["job%d" % si] = repr([None if i is None else job.result(i) for i in idx])
    L = capi.lib()
    L.sk_enum_device_generation.restype = C.c_uint64
    return out, int(L.sk_enum_device_generation())


@pytest.mark.gpu
def test_shutdown_drops_every_buffer_and_the_next_context_starts_clean():
    with open(os.path.join(T.GOLD, "patha_realign_reference.pkl"), "rb") as f:
        gold = pickle.load(f)
    try:
        capi.init(0)
        first, generation = _run_everything(gold)
        assert generation > 0 and _fetch_score(generation) == 0
        dev, pinned = capi.debug_grown_bytes()
        assert dev > 0 and pinned > 0
        gc.collect()  # (pileup stream handles are their owners' to destroy: none of an earlier test's is left waiting for the collector)
        capi.shutdown()
        assert capi.debug_grown_bytes() == (0, 0)
        capi.init(0)
        assert _fetch_score(generation) != 0  # (the run's scores went with the buffers: nothing is read)
        second, _ = _run_everything(gold)
        assert sorted(first) == sorted(second)
        for k in first:
            assert first[k] == second[k], k
    finally:
        capi.init(0)  # (the tests after this one find the library on device 0)
