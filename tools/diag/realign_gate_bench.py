"""time of the realignment gate (sk_realign_gate_dev G0-G4) behind the indel table and candidacy on the windows tools/diag/indel_candidates_bench.py
uses: the seeded synthetic windows of about 8 192 and 16 384 positions at 40x, S = 1 and 8 samples, under the recorded germline configuration, between
device events after a warm-up.  The table, the depth arrays and candidacy are made once on the device and stay there with the key and id counts;
every read's realign range is its own zone widened by 100 positions.  Every result is checked against the model (tests/realign_gate_model.py) run on
the same arrays.  usage: python tools/diag/realign_gate_bench.py [reps [n_pos n_samples]] -> one JSON line (where the time goes, kernel by kernel, for
one shape: rocprofv3 --kernel-trace --stats -- python tools/diag/realign_gate_bench.py 30 16384 8)"""
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
from tests import realign_gate_cases as G  # noqa: E402
from tests import realign_gate_model as GM  # noqa: E402
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
    for n_samples in (1, 8):
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

        run_both()
        # the gate's own arrays
        gate_samples = [dict(reads=[G.read(r["pos"], r["path"], read_len=len(r["code"])) for r in s["reads"]], align_id=None) for s in model_samples]
        for sm in gate_samples:
            for rd in sm["reads"]:
                zone = GM.alignment_zone(rd["pos"], rd["path"], rd["read_len"])
                rd["realign"] = (max(zone[0] - 100, 0), zone[1] + 100)
        want_gate = GM.realign_gate(keys, want, gate_samples, 49)
        gin, gout, gkeep = [], [], []
        for t, sm in zip(keep, gate_samples):
            p = capi.pack_gate_sample(sm["reads"])
            x = dict(read_len=dev(p["read_len"]), realign_begin=dev(p["realign_begin"]), realign_end=dev(p["realign_end"]),
                     reads=torch.zeros((t["n_reads"] + 1) * 12, dtype=torch.uint8, device="cuda"), observed_off=torch.zeros(t["n_reads"] + 2, dtype=torch.int64, device="cuda"),
                     observed=torch.zeros(max(id_cap, 1), dtype=torch.int32, device="cuda"))
            gkeep.append(x)
            gin.append(capi.RealignGateSample(t["n_reads"], 0, ptr(t["pos"]), ptr(t["path_off"]), ptr(t["n_seg"]), ptr(t["path"]), t["n_path"], ptr(x["read_len"]), None,
                                              ptr(x["realign_begin"]), ptr(x["realign_end"])))
            gout.append(capi.RealignGateSampleOut(ptr(x["reads"]), ptr(x["observed_off"]), ptr(x["observed"]), id_cap))
        garr_in, garr_out = (capi.RealignGateSample * n_samples)(*gin), (capi.RealignGateSampleOut * n_samples)(*gout)
        d_gkeys = torch.zeros(max(key_cap, 1) * 48, dtype=torch.uint8, device="cuda")
        d_glogs = torch.zeros(max(key_cap, 1) * n_samples * 16, dtype=torch.uint8, device="cuda")
        d_gtot = torch.zeros(2 + capi.MAX_SAMPLES, dtype=torch.int64, device="cuda")
        g_scratch_bytes = L.sk_realign_gate_scratch_bytes(n_samples, key_cap, id_cap)
        d_g_scratch = torch.zeros(g_scratch_bytes, dtype=torch.uint8, device="cuda")

        def run_gate():
            capi._check(L.sk_realign_gate_dev(n_samples, C.addressof(garr_in), ptr(d_keys), ptr(d_data), ptr(d_ids), ptr(d_tot), key_cap, id_cap, ptr(d_out), ptr(d_rates), 49,
                                              ptr(d_gkeys), ptr(d_glogs), C.addressof(garr_out), ptr(d_gtot), ptr(d_g_scratch), g_scratch_bytes, st))

        ms_gate = timed(run_gate)
        nk, n_ids = (int(x) for x in d_tot.cpu().numpy()[:2])
        assert nk == len(keys)
        res = dict(keys=d_gkeys.cpu().numpy().view(capi.REALIGN_GATE_KEY_DTYPE)[:nk], logs=d_glogs.cpu().numpy().view(capi.REALIGN_GATE_LOG_RATES_DTYPE)[:nk * n_samples],
                   totals=d_gtot.cpu().numpy().tolist(),
                   samples=[dict(reads=x["reads"].cpu().numpy().view(capi.REALIGN_GATE_READ_DTYPE)[:t["n_reads"]], observed_off=x["observed_off"].cpu().numpy()[:t["n_reads"] + 1],
                                 observed=x["observed"].cpu().numpy()) for t, x in zip(keep, gkeep)])
        got = G.device_results(res, n_samples, d_ins.cpu().numpy())
        assert got["keys"] == want_gate["keys"] and got["totals"] == want_gate["totals"]
        for g, w in zip(got["samples"], want_gate["samples"]):
            assert g["reads"] == w["reads"] and g["observed"] == w["observed"]
        result["n_pos_%d_samples_%d" % (n_pos, n_samples)] = dict(reads=sum(len(s["reads"]) for s in dev_samples), positions=n, keys=nk, ids=n_ids, reads_passing=want_gate["totals"][0],
                                                                  reads_undecided=want_gate["totals"][1], observed=sum(want_gate["totals"][2:]),
                                                                  keys_consulted=sum(k["gate_consulted"] for k in want_gate["keys"]), launches=5, ms_gate=ms_gate)
print(json.dumps(result))
