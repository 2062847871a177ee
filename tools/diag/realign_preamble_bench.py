"""time of the realignment preamble (sk_realign_preamble_dev R0-R4) on the windows tools/diag/realign_gate_bench.py uses: the seeded synthetic windows of
about 8 192 and 16 384 positions at 40x, S = 1 and 8 samples, under the recorded germline configuration, between device events after a warm-up.  The
table, candidacy and the gate's outputs are the models' (tests/indel_table_model.py, tests/indel_candidates_model.py, tests/realign_gate_model.py),
uploaded once; every read's realign range is its zone widened by 100 positions.  Every result is checked against the same core on the host
(sk_debug_realign_preamble_host).  Beside it the time one CPU core spends in the job's own preamble for the same passing reads:
sk_realign_job_add_reads with host_threads = 1 and enumeration = 2 (validation, gate, preamble; the search is left pending) on the passing reads,
minus the same call on as many reads that fail the gate (validation and gate alone).
usage: python tools/diag/realign_preamble_bench.py [reps [n_pos n_samples]] -> one JSON line (where the time goes, kernel by kernel, for one shape:
rocprofv3 --kernel-trace --stats -- python tools/diag/realign_preamble_bench.py 30 16384 8 device)"""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from strelka_amd import capi  # noqa: E402
from tests import indel_candidates_model as CM  # noqa: E402
from tests import indel_table_model as T  # noqa: E402
from tests import realign_gate_cases as G  # noqa: E402
from tests import realign_gate_model as GM  # noqa: E402
from tests import realign_preamble_cases as P  # noqa: E402
from tests import region_haplotype_cases as R  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
only = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else None
device_only = len(sys.argv) > 4  # a fifth argument: the device alone (a profiler's run)
capi.init(0)
L = capi.lib()
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
st = torch.cuda.current_stream().cuda_stream


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def window_samples(n_pos, n_samples):
    """as tools/diag/realign_gate_bench.py -> (reference, offset, window, the shared region list, per sample what the models take)"""
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
    model_samples = []
    for c, intake in zip(cases, intakes):
        hap = capi.region_haplotypes(ref, off, c["reads"], c["low"], c["fwd"], regions, win_begin, win_begin + n, 2, intake=intake, opt=opt, raw=True)
        alleles = capi.region_alleles(ref, off, regions, hap, 49, 256, -1, raw=True)
        iat = [0 if k % 11 else 1 for k in range(len(c["reads"]))]
        model_samples.append(dict(reads=c["reads"], fwd=c["fwd"], obs=list(intake["obs"]), align_id=None, iat=iat,
                                  hap=capi.region_haplotype_records(hap["recs"], hap["seq_pool"], hap["support_pool"]),
                                  alleles=capi.region_allele_records(alleles["recs"], alleles["alleles"], alleles["insert_pool"])))
    return ref, off, win_begin, n, regions, model_samples


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


def host_preamble_ms(sc, gate, ins, passes=5):
    """one CPU core: sk_realign_job_add_reads (host_threads = 1, enumeration = 2) on the passing reads minus the same call on as many failing reads, per sample, summed"""
    total = [0.0] * passes
    for s, sm in enumerate(sc["samples"]):
        indels, reads = P.job_inputs(sc, gate, ins, s)
        status = gate["samples"][s]["reads"]["status"][:len(reads)]
        passing = [r for r in range(len(reads)) if status[r] == capi.RGATE_PASS]
        failing = [r for r in range(len(reads)) if status[r] in (capi.RGATE_NO_CANDIDATE, capi.RGATE_OUTSIDE_RANGE)]
        failing = (failing * (len(passing) // max(len(failing), 1) + 1))[:len(passing)] if failing else []
        arrays, keep = [], []
        for chosen in (passing, failing):
            arr = (capi.ReadInput * max(len(chosen), 1))()
            for i, r in enumerate(chosen):
                code, qual, pos, path, fwd, level, sample, realign, observed = reads[r]
                code, qual = np.ascontiguousarray(code, np.uint8), np.ascontiguousarray(qual, np.uint8)
                segs = (capi.PathSeg * max(len(path), 1))(*[capi.PathSeg(t, n) for t, n in path])
                obs = (C.c_int32 * max(len(observed), 1))(*observed)
                keep.append((code, qual, segs, obs))
                arr[i] = capi.ReadInput(code.ctypes.data, qual.ctypes.data, len(code), pos, len(path), segs, int(fwd), level, sample, realign[0], realign[1], len(observed), obs)
            arrays.append((arr, len(chosen)))
        for k in range(passes):
            spent = []
            for arr, n_chosen in arrays:
                job = capi.RealignJob(capi.realign_options(is_haplotyping_enabled=sc["hap"], sample_count=len(sc["samples"]), max_indel_size=sc["max_indel_size"], enumeration=2,
                                                           host_threads=1))
                job.set_reference(sc["ref"], sc["ref_offset"])
                job.set_indels(indels)
                t0 = time.perf_counter()
                first = L.sk_realign_job_add_reads(job._j, arr, n_chosen)
                spent.append((time.perf_counter() - t0) * 1e3)
                assert first == 0, job._err()
            total[k] += spent[0] - spent[1]
    return spread(total)


golden = CM.golden()
cfg = golden["configs"]["germline"]
result = {}
for n_pos in (8192, 16384):
    for n_samples in (1, 8):
        if only and only != (n_pos, n_samples):
            continue
        ref, off, win_begin, n, regions, model_samples = window_samples(n_pos, n_samples)
        copt, sets = CM.config_options(cfg, dict(max_candidate_depth=3 * 40.0 * n_samples, count_towards_depth=[1] * n_samples))
        keys, _ = T.indel_table(ref, off, model_samples, regions, -1)
        depth = [CM.depth_buffers(s["reads"], s["iat"], win_begin, n) for s in model_samples]
        cands, _ = CM.indel_candidates(keys, [s["obs"] for s in model_samples], [d[0] for d in depth], [d[1] for d in depth], win_begin, sets, copt)
        gate_samples = []
        for s in model_samples:
            reads = []
            for r, fwd in zip(s["reads"], s["fwd"]):
                rd = G.read(r["pos"], r["path"], read_len=len(r["code"]))
                zone = GM.alignment_zone(rd["pos"], rd["path"], rd["read_len"])
                reads.append(dict(rd, realign=(max(zone[0] - 100, 0), zone[1] + 100), seq="".join(P.CODE_CHAR[int(c)] for c in r["code"]), fwd=bool(fwd), n_code=len(r["code"])))
            gate_samples.append(dict(reads=reads, align_id=None))
        sc = dict(name="n_pos_%d_samples_%d" % (n_pos, n_samples), ref=ref, ref_offset=off, max_indel_size=49, hap=cfg["is_haplotyping_enabled"], keys=keys, cands=cands,
                  samples=gate_samples, expect={})
        gate, ins, want_gate = P.model_gate(sc)
        want = P.preamble(sc, True, gate, ins)
        ps, pp = P.packed(sc)
        nk, n_pass = len(keys), want_gate["totals"][0]
        key_cap, record_cap = nk + 1, n_pass + 1
        keep, a_in, a_gate, a_pre, statuses = [], [], [], [], []
        for p, q, g in zip(ps, pp, gate["samples"]):
            d = {f: dev(p[f]) for f in ("pos", "path_off", "n_seg", "path", "read_len", "realign_begin", "realign_end")}
            e = dict(reads=dev(g["reads"]), observed_off=dev(g["observed_off"]), observed=dev(g["observed"]), read_code=dev(q["read_code"]), read_off=dev(q["read_off"]),
                     fwd=dev(q["is_fwd_strand"]), status=torch.zeros(p["n_reads"] + 1, dtype=torch.uint8, device="cuda"))
            keep.append((d, e))
            statuses.append(e["status"])
            a_in.append(capi.realign_gate_sample_struct(dict(p, align_id=None, **d), ptr=lambda x: x.data_ptr()))
            a_gate.append(capi.RealignGateSampleOut(e["reads"].data_ptr(), e["observed_off"].data_ptr(), e["observed"].data_ptr(), g["observed_cap"]))
            a_pre.append(capi.RealignPreambleSample(e["read_code"].data_ptr(), e["read_off"].data_ptr(), q["code_cap"], e["fwd"].data_ptr(), e["status"].data_ptr()))
        arr_in, arr_gate, arr_pre = (capi.RealignGateSample * n_samples)(*a_in), (capi.RealignGateSampleOut * n_samples)(*a_gate), (capi.RealignPreambleSample * n_samples)(*a_pre)
        d_keys = dev(np.concatenate([gate["keys"], np.zeros(1, capi.REALIGN_GATE_KEY_DTYPE)]))
        d_tot, d_ins, d_ref = dev(np.array([nk, 0, 0, 0], np.int64)), dev(np.concatenate([ins, np.zeros(1, np.uint8)])), dev(np.frombuffer(ref.encode() + b"\0", np.uint8))
        d_rec, d_src = torch.zeros(record_cap * 784, dtype=torch.uint8, device="cuda"), torch.zeros(record_cap * 8, dtype=torch.uint8, device="cuda")
        d_cons, d_ptot = torch.zeros(key_cap, dtype=torch.uint8, device="cuda"), torch.zeros(capi.RPRE_N_TOTALS, dtype=torch.int64, device="cuda")
        scratch_bytes = capi.realign_preamble_scratch_bytes(n_samples, key_cap, record_cap)
        d_scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")

        def run_preamble():
            capi.realign_preamble_dev(n_samples, C.addressof(arr_in), C.addressof(arr_gate), C.addressof(arr_pre), d_keys.data_ptr(), d_tot.data_ptr(), key_cap, d_ins.data_ptr(),
                                      len(ins), d_ref.data_ptr(), off, len(ref), 49, d_rec.data_ptr(), d_src.data_ptr(), record_cap, d_cons.data_ptr(), d_ptot.data_ptr(),
                                      d_scratch.data_ptr(), scratch_bytes, st)

        ms = timed(run_preamble)
        n_rec = want["totals"][0]
        assert d_ptot.cpu().numpy().tolist() == want["totals"]
        assert d_rec.cpu().numpy().view(capi.REALIGN_PREPARED_READ_DTYPE)[:n_rec].tobytes() == want["records"][:n_rec].tobytes()
        assert d_src.cpu().numpy().view(capi.REALIGN_PREPARED_SOURCE_DTYPE)[:n_rec].tobytes() == want["source"][:n_rec].tobytes()
        assert (d_cons.cpu().numpy()[:nk] == want["consulted"][:nk]).all()
        assert all((s.cpu().numpy()[:len(w)] == w).all() for s, w in zip(statuses, want["status"]))
        result[sc["name"]] = dict(reads=sum(len(s["reads"]) for s in gate_samples), keys=nk, reads_passing=n_pass, records=n_rec,
                                  by_status={capi.RPRE_NAMES[i]: v for i, v in enumerate(want["totals"][1:]) if v}, keys_consulted=int(want["consulted"][:nk].sum()),
                                  launches=5, ms_preamble=ms, ms_host_preamble_one_core=None if device_only else host_preamble_ms(sc, gate, ins))
print(json.dumps(result))
