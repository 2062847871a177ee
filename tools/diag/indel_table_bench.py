"""time of the indel table (sk_indel_table_dev, T0-T4) on the seeded synthetic windows of about 8 192 and 16 384 positions at 40x
(tests/region_haplotype_cases.seeded_window), S = 1, 2 and 8 samples (each the window's reads without every eighth one, a different eighth per sample),
between device events after a warm-up.  The inputs are what the chain's host entries leave (sk_read_intake -> sk_sync_active_regions over the samples -> per sample
sk_region_haplotypes -> sk_region_alleles), uploaded once.  Every result is checked against the model (tests/indel_table_model.py) run on
the same arrays.  usage: python tools/diag/indel_table_bench.py [reps [n_pos n_samples]] -> one JSON line; with a shape named only that one runs
(for a kernel trace of its own: rocprofv3 --kernel-trace --stats -- python tools/diag/indel_table_bench.py 30 16384 8)"""
import ctypes as C
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from strelka_amd import capi  # noqa: E402
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
    """-> (reference, offset, the shared region list, per sample what capi.indel_table takes and what the model takes)"""
    base = R.seeded_window(n_pos * 40 // 100, 9100 + n_pos)
    ref, off, win_begin, n = base["ref"], base["ref_offset"], base["win_begin"], base["n_pos"]
    cases = []
    for s in range(n_samples):  # one reference for all: sample s is the window without every eighth read, counted from s (35x each)
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
    return ref, off, regions, dev_samples, model_samples


result = {}
for n_pos in (8192, 16384):
    for n_samples in (1, 2, 8):
        if only and only != (n_pos, n_samples):
            continue
        ref, off, regions, dev_samples, model_samples = window_samples(n_pos, n_samples)
        want, want_totals = T.indel_table(ref, off, model_samples, regions, -1)
        m = len(regions)
        reg = np.zeros(m + 1, capi.ACTIVE_REGION_DTYPE)
        for i, (b, e) in enumerate(regions):
            reg[i] = (b, e, 0)
        keep, structs, tot = [], [], dict(n_obs=0, n_alleles=0, n_support=0, n_bases=0, n_ins=0)
        for s in dev_samples:
            sm, arrays, sizes = capi.pack_indel_table_sample(s, m)
            t = {k: (None if a is None else dev(np.concatenate([a, np.zeros(1, a.dtype)]).view(np.uint8))) for k, a in arrays.items()}
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

        def run():
            capi._check(L.sk_indel_table_dev(n_samples, C.addressof(arr), ptr(d_ref), off, len(ref), ptr(d_reg), ptr(d_n), m, -1, expand_cap, ptr(d_keys), key_cap, ptr(d_data),
                                             ptr(d_ids), id_cap, ptr(d_ins), ins_cap, ptr(d_tot), ptr(d_scratch), scratch_bytes, st))

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
        totals = d_tot.cpu().numpy()
        nk = int(totals[0])
        got = capi.indel_table_records(d_keys.cpu().numpy()[:nk * 56].view(capi.INDEL_TABLE_KEY_DTYPE), d_data.cpu().numpy()[:nk * n_samples * 64].view(capi.INDEL_TABLE_SAMPLE_DATA_DTYPE),
                                       d_ids.cpu().numpy().view(np.uint32)[:int(totals[1])], d_ins.cpu().numpy()[:int(totals[2])], n_samples)
        assert got == want and totals.tolist() == want_totals
        passes, w = 0, 1024
        while w < expand_cap:
            passes, w = passes + 1, 2 * w
        result["n_pos_%d_samples_%d" % (n_pos, n_samples)] = dict(reads=sum(len(s["reads"]) for s in dev_samples), regions=m, observations=tot["n_obs"], expanded_records=expand_cap,
                                                                  keys=nk, ids=int(totals[1]), pending_pairs=int(totals[3]), launches=5 + passes, ms=spread(ms))
print(json.dumps(result))
