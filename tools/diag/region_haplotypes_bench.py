"""time of the region-haplotype kernels (sk_region_haplotypes_dev: H0-H3) between device events, after a warm-up:
  * on the regions of the tests' seeded window of 2 200 reads (the results checked against tests/haplotype_model.py),
  * on a bulk case of 2^16 reads with variants at the same density (a prefix of its regions checked against the model),
  * the whole chain sk_read_intake_dev -> sk_ref_anchors_dev -> sk_active_regions_dev -> sk_region_haplotypes_dev on one stream for the
    seeded window,
and, when the golden driver has been built (tools/golden/region_haplotypes_driver.cpp), the reference's own getReadSegments +
generateHaplotypesWithCounting's grouping + selectHaplotypes on the seeded window's regions on one core (its TIME command; the window
goes to the driver in pieces of fewer than 1 000 positions and reads, which is what its ring holds).
usage: python tools/diag/region_haplotypes_bench.py [reps] [out.txt] -> one JSON line, and the table in out.txt"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from strelka_amd import capi  # noqa: E402
from tests import haplotype_model as H  # noqa: E402
from tests import intake_model as M  # noqa: E402
from tests import region_haplotype_cases as R  # noqa: E402
from tests import test_region_haplotypes as T  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
capi.init(0)
L = capi.lib()
p = lambda t: C.c_void_p(t.data_ptr())
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


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


def region_array(regions):
    a = np.zeros(max(len(regions), 1), capi.ACTIVE_REGION_DTYPE)
    for i, (b, e) in enumerate(regions):
        a[i] = (b, e, 0)
    return a


def statuses(recs):
    return dict(regions=len(recs), counted=sum(1 for r in recs if r["status"] == H.COUNTED), two_or_more=sum(1 for r in recs if len(r["haps"]) >= 2),
                declined=sum(1 for r in recs if r["status"] == H.DECLINED), selected=sum(len(r["haps"]) for r in recs))


result = {}

# ---- the seeded window: haplotypes alone, then the whole chain ------------------------------------------------------------------------------------------
c, intake_m, anchor_m, regions_m, want = R.seeded_window_model()
n, win_begin, n_pos = len(c["reads"]), c["win_begin"], c["n_pos"]
host_intake = capi.read_intake(c["ref"], c["ref_offset"], c["reads"], c["low"], win_begin, n_pos)
n_regions = len(c["regions"])
d = T._dev_upload(c, n_regions, host_intake)
d_regions, d_n = dev(region_array(c["regions"]).view(np.int32)), dev(np.array([n_regions], np.int32))
torch.cuda.synchronize()
t_hap = timed(lambda: T._dev_launch(c, d, d_regions, d_n, st))
got = T._dev_records(d, n_regions)
assert got == want
result["window_2200_reads"] = dict(reads=n, positions=n_pos, haplotypes_ms=t_hap, **statuses(want))

region_cap = capi.active_regions_bound(n_pos)
dc = T._dev_upload(c, region_cap)
n_segs = dc["n_segs"]
cap = capi.read_intake_obs_bound(n_segs)
d_reads = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
dc["obs_off"] = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
dc["obs"] = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
d_sites = torch.zeros(n_pos, dtype=torch.int64, device="cuda")
d_cand = torch.zeros(n_pos, dtype=torch.uint8, device="cuda")
scratch_bytes = L.sk_read_intake_scratch_bytes(n, n_segs, n_pos)
d_scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
d_anchor = torch.zeros(n_pos, dtype=torch.uint8, device="cuda")
d_state_in = dev(capi.ar_state_initial().view(np.int32))
d_state_out = torch.zeros(6, dtype=torch.int32, device="cuda")
d_chain_regions = torch.zeros(region_cap * 3, dtype=torch.int32, device="cuda")
d_chain_n = torch.zeros(1, dtype=torch.int32, device="cuda")
opt = capi.intake_options()
t = dc["t"]


def chain():
    capi._check(L.sk_read_intake_dev(p(dc["ref"]), c["ref_offset"], len(c["ref"]), n, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]), C.byref(opt),
                                     win_begin, n_pos, p(d_reads), p(dc["obs_off"]), p(dc["obs"]), cap, p(d_sites), p(d_cand), p(d_scratch), scratch_bytes, st))
    capi._check(L.sk_ref_anchors_dev(p(dc["ref"]), c["ref_offset"], len(c["ref"]), win_begin + 1, None, win_begin, n_pos, p(d_anchor), 0, None, None, st))
    capi._check(L.sk_active_regions_dev(win_begin, n_pos, p(d_sites), p(d_cand), p(d_anchor), p(d_state_in), p(d_state_out), p(d_chain_regions), region_cap,
                                        p(d_chain_n), st))
    T._dev_launch(c, dc, d_chain_regions, d_chain_n, st)


torch.cuda.synchronize()
t_chain = timed(chain)
assert int(d_chain_n.cpu()[0]) == n_regions and T._dev_records(dc, n_regions) == want
result["window_2200_reads"]["chain_of_four_ms"] = t_chain

# ---- the bulk case: 2^16 reads --------------------------------------------------------------------------------------------------------------------------
big = R.seeded_window(n_reads=1 << 16, seed=9200)
bn, b_begin, b_pos = len(big["reads"]), big["win_begin"], big["n_pos"]
b_intake = capi.read_intake(big["ref"], big["ref_offset"], big["reads"], big["low"], b_begin, b_pos)
b_anchor, _ = capi.ref_anchors(big["ref"], big["ref_offset"], b_begin + 1, None, b_begin, b_pos)
b_regions, _ = capi.active_regions(b_begin, b_intake["sites"], b_intake["is_candidate"], b_anchor)
big = dict(big, regions=[(int(r["begin"]), int(r["end"])) for r in b_regions])
bd = T._dev_upload(big, len(b_regions), b_intake)
bd_regions, bd_n = dev(np.ascontiguousarray(b_regions).view(np.int32)), dev(np.array([len(b_regions)], np.int32))
torch.cuda.synchronize()
t_big = timed(lambda: T._dev_launch(big, bd, bd_regions, bd_n, st))
b_got = T._dev_records(bd, len(b_regions))
# a prefix against the model: the first 3 000 reads (their indices are their own) and the regions that end before the 3 000th begins
prefix = 3000
cut = int(big["reads"][prefix]["pos"]) - 5
head = [r for r in big["regions"] if r[1] < cut]
sub = dict(big, reads=big["reads"][:prefix], low=big["low"][:prefix], fwd=big["fwd"][:prefix], regions=head)
assert len(head) >= 20 and b_got[:len(head)] == R.model(sub)
result["bulk_65536_reads"] = dict(reads=bn, positions=b_pos, haplotypes_ms=t_big, checked_regions=len(head), **statuses(b_got))

# ---- the reference on one core --------------------------------------------------------------------------------------------------------------------------
driver = os.path.join("oracle", "_ref", "bin", "region_haplotypes_driver")
if os.path.exists(driver):
    seconds, pieces, regions_timed = 0.0, 0, 0
    k = 0
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
        lines += ["REGION %d %d 2" % g for g in piece] + ["TIME 200"]
        out = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True, universal_newlines=True).stdout
        seconds += json.loads(out)["seconds_per_pass"]
        pieces += 1
        regions_timed += len(piece)
        k += len(piece)
    result["reference_one_core"] = dict(regions=regions_timed, pieces=pieces, ms=seconds * 1e3)
else:
    result["reference_one_core"] = "not measured (tools/golden/region_haplotypes_driver.cpp not built)"

print(json.dumps(result))
if out_path:
    f3 = lambda s: "%.4f [%.4f %.4f]" % (s["median"], s["min"], s["max"])
    w, b = result["window_2200_reads"], result["bulk_65536_reads"]
    with open(out_path, "w") as f:
        f.write("# tools/diag/region_haplotypes_bench.py %d on one MI355X: sk_region_haplotypes_dev (H0-H3: four launches and a 256-byte memset) between device events,\n"
                "# 3 warm-up calls, %d repetitions; ms as median [min max].  One visit.\n" % (reps, reps))
        f.write("shape                                                    regions  counted  >=2 haplotypes  declined  haplotypes alone             chain of four (intake, anchors, walk, haplotypes)\n")
        f.write("seeded window: %5d reads, %6d positions              %7d  %7d  %14d  %8d  %-28s %s\n" % (w["reads"], w["positions"], w["regions"], w["counted"], w["two_or_more"],
                                                                                                              w["declined"], f3(w["haplotypes_ms"]), f3(w["chain_of_four_ms"])))
        f.write("bulk: %5d reads, %7d positions                      %7d  %7d  %14d  %8d  %-28s -\n" % (b["reads"], b["positions"], b["regions"], b["counted"], b["two_or_more"],
                                                                                                          b["declined"], f3(b["haplotypes_ms"])))
        f.write("# the window's records equal tests/haplotype_model.py's; of the bulk case the first %d regions were compared with it\n" % b["checked_regions"])
        ref = result["reference_one_core"]
        if isinstance(ref, dict):
            f.write("# the reference's own getReadSegments + grouping + selectHaplotypes on the seeded window's %d regions on one core of the same machine, timed inside\n"
                    "# tools/golden/region_haplotypes_driver.cpp (TIME, %d pieces of fewer than 1 000 positions and reads): %.3f ms\n" % (ref["regions"], ref["pieces"], ref["ms"]))
        else:
            f.write("# the reference on one core: %s\n" % ref)
