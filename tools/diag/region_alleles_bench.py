"""time of the chain's last stage (sk_region_alleles_dev: A0, A1, the aligner, A2-A4) between device events, after a warm-up, on the regions of
the tests' seeded window of 2 200 reads (the records checked against tests/alleles_model.py), and the reference's own
processSelectedHaplotypes over the same regions on one core (tools/golden/region_alleles_driver.cpp, its TIME command; the window goes to
the driver in pieces of fewer than 1 000 positions and reads, which is what its ring holds).
usage: python tools/diag/region_alleles_bench.py gpu [reps] out.json     on the device
       python tools/diag/region_alleles_bench.py ref out.json            where the golden driver has been built
       python tools/diag/region_alleles_bench.py table gpu.json ref.json out.txt"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, ".")
from tests import intake_model as M  # noqa: E402
from tests import region_haplotype_cases as R  # noqa: E402

MAX_HAP_LEN = 256
mode = sys.argv[1]

if mode == "gpu":
    import torch
    from strelka_amd import capi
    from tests import alleles_model as A
    reps, out_path = int(sys.argv[2]), sys.argv[3]
    capi.init(0)
    L = capi.lib()
    c, _, _, _, hap_want = R.seeded_window_model()
    n_regions = len(c["regions"])
    hap = capi.region_haplotypes(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], c["regions"], c["buf_begin"], c["buf_end"], c["ploidy"], raw=True)
    want, _ = A.region_alleles(c["ref"], c["ref_offset"], c["regions"], hap_want, c["max_indel_size"], MAX_HAP_LEN, -1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    regions = np.zeros(n_regions, capi.ACTIVE_REGION_DTYPE)
    for i, (b, e) in enumerate(c["regions"]):
        regions[i] = (b, e, 0)
    allele_cap, insert_cap = capi.region_alleles_bounds(n_regions, MAX_HAP_LEN)
    scratch_bytes = L.sk_region_alleles_scratch_bytes(n_regions, MAX_HAP_LEN)
    d = dict(ref=dev(np.frombuffer(c["ref"].encode(), np.uint8).copy()), regions=dev(regions.view(np.int32)), n=dev(np.array([n_regions], np.int32)),
             hap=dev(hap["recs"].view(np.uint8)), seq=dev(np.concatenate([hap["seq_pool"], np.zeros(8, np.uint8)])),
             recs=torch.zeros(n_regions * 72, dtype=torch.uint8, device="cuda"), alleles=torch.zeros(allele_cap * 56, dtype=torch.uint8, device="cuda"),
             ins=torch.zeros(insert_cap, dtype=torch.uint8, device="cuda"), totals=torch.zeros(2, dtype=torch.int64, device="cuda"),
             prev=torch.zeros(1, dtype=torch.int32, device="cuda"), scratch=torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda"))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        capi._check(L.sk_region_alleles_dev(p(d["ref"]), c["ref_offset"], len(c["ref"]), p(d["regions"]), p(d["n"]), n_regions, p(d["hap"]), p(d["seq"]), len(hap["seq_pool"]),
                                            c["max_indel_size"], MAX_HAP_LEN, -1, p(d["recs"]), p(d["alleles"]), allele_cap, p(d["ins"]), insert_cap, p(d["totals"]),
                                            p(d["prev"]), p(d["scratch"]), scratch_bytes, st))
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
    totals = d["totals"].cpu().numpy()
    got = capi.region_allele_records(d["recs"].cpu().numpy().view(capi.REGION_ALLELES_DTYPE), d["alleles"].cpu().numpy().view(capi.REGION_ALLELE_DTYPE)[:int(totals[0])],
                                     d["ins"].cpu().numpy()[:int(totals[1])])
    assert got == want
    res = dict(reps=reps, reads=len(c["reads"]), positions=c["n_pos"], regions=n_regions, with_alternates=sum(1 for r in want if r["n_alt"]),
               alternates=sum(r["n_alt"] for r in want), alleles=int(totals[0]), ms=dict(median=statistics.median(ms), min=min(ms), max=max(ms)))
    with open(out_path, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))
elif mode == "ref":
    out_path = sys.argv[2]
    driver = os.path.join("oracle", "_ref", "bin", "region_alleles_driver")
    c, _, _, _, _ = R.seeded_window_model()
    seconds, pieces, regions_timed, counted, k = 0.0, 0, 0, 0, 0
    regs = c["regions"]
    while k < len(regs):
        piece = [regs[k]]
        while k + len(piece) < len(regs) and regs[k + len(piece)][1] - piece[0][0] < 700:
            piece.append(regs[k + len(piece)])
        lo, hi = piece[0][0] - 120, piece[-1][1] + 120
        keep = [i for i, r in enumerate(c["reads"]) if lo <= r["pos"] and r["pos"] + 130 <= hi]
        assert len(keep) < 1000 and hi - lo < 1000
        lines = ["REF %d %s" % (c["ref_offset"], c["ref"]), "OPT %d" % c["max_indel_size"], "BUF %d %d" % (lo, hi)]
        for i in keep:
            r = c["reads"][i]
            lines.append("READ %d %d %d %s %d %s" % (r["pos"], c["low"][i], c["fwd"][i], M.read_string(r["code"], 0, len(r["code"])), len(r["path"]),
                                                     " ".join("%d %d" % (a, b) for a, b in r["path"])))
        prev_end = regs[k - 1][1] if k else -1
        for g in piece:
            lines.append("REGION %d %d 2 %d" % (g[0], g[1], prev_end))
            prev_end = g[1]
        lines.append("TIME 200")
        out = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True, universal_newlines=True).stdout
        doc = json.loads(out)
        seconds += doc["seconds_per_pass"]
        counted += doc["counted"]
        pieces += 1
        regions_timed += len(piece)
        k += len(piece)
    res = dict(regions=regions_timed, counted=counted, pieces=pieces, repeats=200, ms=seconds * 1e3)
    with open(out_path, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))
else:
    with open(sys.argv[2]) as f:
        g = json.load(f)
    with open(sys.argv[3]) as f:
        r = json.load(f)
    with open(sys.argv[4], "w") as f:
        f.write("# tools/diag/region_alleles_bench.py gpu %d on one MI355X: sk_region_alleles_dev (A0, A1, the aligner over a grid of 2 x regions, A2, A3, A4: six launches)\n"
                "# between device events, 3 warm-up calls, %d repetitions, max_hap_len %d; ms as median [min max].  One visit.\n" % (g["reps"], g["reps"], MAX_HAP_LEN))
        f.write("shape                                                    regions  with alternates  alternates  alleles  alleles stage\n")
        f.write("seeded window: %5d reads, %6d positions              %7d  %15d  %10d  %7d  %.4f [%.4f %.4f]\n" % (g["reads"], g["positions"], g["regions"], g["with_alternates"],
                                                                                                               g["alternates"], g["alleles"], g["ms"]["median"], g["ms"]["min"],
                                                                                                               g["ms"]["max"]))
        f.write("# the window's records equal tests/alleles_model.py's\n")
        f.write("# the reference's own processSelectedHaplotypes (the aligner, the walk, the buffers' insertions) on the seeded window's %d regions (%d counted) on one core of the\n"
                "# machine the vectors were recorded on, timed inside tools/golden/region_alleles_driver.cpp (TIME %d, %d pieces of fewer than 1 000 positions and reads; the selection and the\n"
                "# buffers' construction outside the clock): %.3f ms.  Not the device's host: the two figures are one visit each and not a ratio.\n"
                % (r["regions"], r["counted"], r["repeats"], r["pieces"], r["ms"]))
