"""time of indel candidacy (sk_read_depth_dev D0-D3 per sample, sk_indel_candidates_dev C0-C2) behind the indel table on the windows
tools/diag/indel_table_bench.py uses: the seeded synthetic windows of about 8 192 and 16 384 positions at 40x, S = 1, 2 and 8 samples, under
the recorded germline configuration (rate sets, papprox and log factor of tests/golden/indel_candidates), between device events after a
warm-up.  The table is made once by sk_indel_table_dev and stays on the device with its key count.  Every result is checked against the model
(tests/indel_candidates_model.py) run on the same arrays.  usage: python tools/diag/indel_candidates_bench.py [reps [n_pos n_samples]] -> one
JSON line (for a kernel trace of one shape: rocprofv3 --kernel-trace --stats -- python tools/diag/indel_candidates_bench.py 30 16384 8)"""
import ctypes as C
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from strelka_amd import capi  # noqa: E402
from tests import indel_candidates_cases as K  # noqa: E402
from tests import indel_candidates_model as CM  # noqa: E402
from tests import indel_table_model as T  # noqa: E402
from tests import region_haplotype_cases as R  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
only = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else None
capi.init(0)
L = capi.lib()
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
ptr = lambda t: None if t is None else t.data_ptr()
st = torch.cuda.current_stream().cuda_stream


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def window_samples(n_pos, n_samples):
    """as tools/diag/indel_table_bench.py -> (reference, offset, window, the shared region list, per sample what capi.indel_table takes and what the model takes)"""
    base = R.seeded_window(n_pos * 40 // 100, 9100 + n_pos)
    ref, off, win_begin, n = base["ref"], base["ref_offset"], base["win_begin"], base["n_pos"]
    cases = []
    for s in range(n_samples):
        keep = [k for k in range(len(base["reads"])) if n_samples == 1 or k % 8 != s]
        cases.append(dict(reads=[base["reads"][k] for k in keep], low=[base["low"][k] for k in keep], fwd=[base["fwd"][k] for k in keep]))
    opt = capi.intake_options()
    intakes = [capi.read_intake(ref, off, c["reads"], c["low"], win_begin, n, opt) for c in cases]
    anchor, _ = capi.ref_anchors(ref, off, win_begin + 1, None, win_begin, n)
    sync, _, _ = capi.sync_active_regions(win_begin, np.array([i["sites"] for i in intakes]), np.array([i["is_candidate"] for i in intakes]), anchor, do_clear=True,
                                          buf_begin=[win_begin] * n_samples, buf_end=[win_begin + n] * n_samples)
    regions = [(int(g["begin"]), int(g["end"])) for g in sync]
    dev_samples, model_samples = [], []
    for c, intake in zip(cases, intakes):
        hap = capi.region_haplotypes(ref, off, c["reads"], c["low"], c["fwd"], regions, win_begin, win_begin + n, 2, intake=intake, opt=opt, raw=True)
        alleles = capi.region_alleles(ref, off, regions, hap, 49, 256, -1, raw=True)
        iat = [0 if k % 11 else 1 for k in range(len(c["reads"]))]
        dev_samples.append(dict(reads=c["reads"], intake=intake, align_id=None, iat=iat, haplotypes=hap, alleles=alleles))
        model_samples.append(dict(reads=c["reads"], obs=list(intake["obs"]), align_id=None, iat=iat, hap=capi.region_haplotype_records(hap["recs"], hap["seq_pool"], hap["support_pool"]),
                                  alleles=capi.region_allele_records(alleles["recs"], alleles["alleles"], alleles["insert_pool"])))
    return ref, off, win_begin, n, regions, dev_samples, model_samples


def timed(run):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return spread(ms)


golden = CM.golden()
cfg = golden["configs"]["germline"]
result = {}
for n_pos in (8192, 16384):
    for n_samples in (1, 2, 8):
        if only and only != (n_pos, n_samples):
            continue
        ref, off, win_begin, n, regions, dev_samples, model_samples = window_samples(n_pos, n_samples)
        copt, sets = CM.config_options(cfg, dict(max_candidate_depth=3 * 40.0 * n_samples, count_towards_depth=[1] * n_samples))
        keys, _ = T.indel_table(ref, off, model_samples, regions, -1)
        depth = [CM.depth_buffers(s["reads"], s["iat"], win_begin, n) for s in model_samples]
        want, want_totals = CM.indel_candidates(keys, [s["obs"] for s in model_samples], [d[0] for d in depth], [d[1] for d in depth], win_begin, sets, copt)
        m = len(regions)
        reg = np.zeros(m + 1, capi.ACTIVE_REGION_DTYPE)
        for i, (b, e) in enumerate(regions):
            reg[i] = (b, e, 0)
        keep, structs, tot = [], [], dict(n_obs=0, n_alleles=0, n_support=0, n_bases=0, n_ins=0)
        for s in dev_samples:
            sm, arrays, sizes = capi.pack_indel_table_sample(s, m)
            t = {k: (None if a is None else dev(np.concatenate([a, np.zeros(1, a.dtype)]).view(np.uint8))) for k, a in arrays.items()}
            path_off, n_seg, path, pos = capi.pack_paths(s["reads"])
            t.update(path_off=dev(path_off), n_seg=dev(n_seg), path=dev(path), pos=dev(pos), n_path=len(path) - 1, n_reads=sm.n_reads, obs_cap=sm.obs_cap,
                     depth1=torch.zeros(n + 1, dtype=torch.int32, device="cuda"), depth2=torch.zeros(n + 1, dtype=torch.int32, device="cuda"))
            keep.append(t)
            structs.append(capi.IndelTableSample(sm.n_reads, 0, ptr(t["read_off"]), ptr(t["code"]), ptr(t["obs_off"]), ptr(t["obs"]), sm.obs_cap, ptr(t["align_id"]), ptr(t["iat"]),
                                                 ptr(t["hap"]), ptr(t["support"]), sm.support_cap, ptr(t["recs"]), ptr(t["alleles"]), sm.allele_cap, ptr(t["ins"]), sm.insert_cap))
            for k in tot:
                tot[k] += sizes[k]
        arr = (capi.IndelTableSample * n_samples)(*structs)
        key_cap, id_cap, ins_cap = capi.indel_table_bounds(tot["n_obs"], tot["n_alleles"], tot["n_support"], tot["n_bases"], tot["n_ins"])
        expand_cap = tot["n_obs"] + tot["n_alleles"] + tot["n_support"]
        d_ref, d_reg, d_n = dev(np.frombuffer(ref.encode(), np.uint8).copy()), dev(reg.view(np.int32)), dev(np.array([m], np.int32))
        d_keys = torch.zeros(max(key_cap, 1) * 56, dtype=torch.uint8, device="cuda")
        d_data = torch.zeros(max(key_cap, 1) * n_samples * 64, dtype=torch.uint8, device="cuda")
        d_ids = torch.zeros(max(id_cap, 1), dtype=torch.int32, device="cuda")
        d_ins = torch.zeros(max(ins_cap, 1), dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
        scratch_bytes = L.sk_indel_table_scratch_bytes(n_samples, expand_cap, m)
        d_scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
        capi._check(L.sk_indel_table_dev(n_samples, C.addressof(arr), ptr(d_ref), off, len(ref), ptr(d_reg), ptr(d_n), m, -1, expand_cap, ptr(d_keys), key_cap, ptr(d_data),
                                         ptr(d_ids), id_cap, ptr(d_ins), ins_cap, ptr(d_tot), ptr(d_scratch), scratch_bytes, st))
        depth_scratch_bytes = L.sk_read_depth_scratch_bytes(n)
        d_depth_scratch = torch.zeros(depth_scratch_bytes, dtype=torch.uint8, device="cuda")
        d_sets = dev(K.rate_set_arrays(sets).view(np.uint8))
        d_out = torch.zeros(max(key_cap, 1) * 8, dtype=torch.uint8, device="cuda")
        d_rates = torch.zeros(max(key_cap, 1) * n_samples * 32, dtype=torch.uint8, device="cuda")
        d_ctot = torch.zeros(2, dtype=torch.int64, device="cuda")
        c_scratch_bytes = L.sk_indel_candidates_scratch_bytes()
        d_c_scratch = torch.zeros(c_scratch_bytes, dtype=torch.uint8, device="cuda")
        carr = (capi.IndelCandidateSample * n_samples)(*[capi.IndelCandidateSample(t["n_reads"], 0, ptr(t["obs_off"]), ptr(t["obs"]), t["obs_cap"], ptr(t["depth1"]), ptr(t["depth2"]))
                                                         for t in keep])
        o = K.capi_options(copt)

        def run_depth():
            for t in keep:
                capi._check(L.sk_read_depth_dev(t["n_reads"], ptr(t["path_off"]), ptr(t["n_seg"]), ptr(t["path"]), t["n_path"], ptr(t["pos"]), ptr(t["iat"]), win_begin, n,
                                                ptr(t["depth1"]), ptr(t["depth2"]), ptr(d_depth_scratch), depth_scratch_bytes, st))

        def run_candidates():
            capi._check(L.sk_indel_candidates_dev(n_samples, C.addressof(carr), win_begin, n, ptr(d_keys), ptr(d_data), ptr(d_tot), key_cap, ptr(d_sets), C.addressof(o), ptr(d_out),
                                                  ptr(d_rates), ptr(d_ctot), ptr(d_c_scratch), c_scratch_bytes, st))

        def run_both():
            run_depth()
            run_candidates()

        ms_depth, ms_cand, ms_both = timed(run_depth), timed(run_candidates), timed(run_both)
        nk = int(d_tot.cpu().numpy()[0])
        assert nk == len(keys)
        for t, (w1, w2) in zip(keep, depth):
            assert t["depth1"].cpu().numpy().view(np.uint32)[:n].tolist() == w1.tolist() and t["depth2"].cpu().numpy().view(np.uint32)[:n].tolist() == w2.tolist()
        got = K.device_results(dict(out=d_out.cpu().numpy().view(capi.INDEL_CANDIDATE_DTYPE)[:nk], rates=d_rates.cpu().numpy().view(capi.INDEL_ERROR_RATES_DTYPE)[:nk * n_samples]), n_samples)
        assert got == want and d_ctot.cpu().numpy().tolist() == want_totals
        result["n_pos_%d_samples_%d" % (n_pos, n_samples)] = dict(reads=sum(len(s["reads"]) for s in dev_samples), positions=n, keys=nk, key_cap=key_cap, observations=tot["n_obs"],
                                                                  candidates=want_totals[0], undecided=want_totals[1], launches_depth=4 * n_samples, launches_candidates=3,
                                                                  ms_depth=ms_depth, ms_candidates=ms_cand, ms_both=ms_both)
print(json.dumps(result))
