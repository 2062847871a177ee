"""time of the active-region kernels: sk_ref_anchors_dev (AR1) and sk_active_regions_dev (AR2) between device events, after a warm-up,
on one pileup-stream window of 8 192 positions (a window right at a region's start, so that the head kernel runs, and one 1 000 past
it), AR1 alone on 2^26 positions, and the span rows of 4 positions (one inside a 600-base homopolymer).  The window's results are
checked against the model (tests/anchor_model.py); the large shape is a periodic reference, checked period against period.  When the
golden driver has been built (tools/golden/active_region_driver.cpp), the reference's own finder is timed over the window's sequence
and over 2^22 positions on one core.  usage: python tools/diag/active_region_bench.py [reps] -> one JSON line"""
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
from tests import active_region_cases as R  # noqa: E402
from tests import anchor_model as A  # noqa: E402
from tests import intake_cases as K  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
capi.init(0)
L = capi.lib()
WINDOW = 8192
OFF = 1000
p = lambda t: C.c_void_p(t.data_ptr())
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


result = {}
rng = np.random.default_rng(8802)
ref = K.repeat_rich_reference(WINDOW + 1400, rng)
ref = ref[:3000] + "A" * 600 + "C" + ref[3601:]
sites = R.walk_sites(WINDOW, rng, 0.004)  # a few dozen candidates per window
d_ref = torch.from_numpy(np.frombuffer(ref.encode(), np.uint8).copy()).cuda()

for name, win_begin in (("window_8192_at_region_start", OFF), ("window_8192", OFF + 1000)):
    init_pos = OFF + 1  # the detector's first call of the region
    depth, cand, anchor = R.walk_flags(ref, OFF, win_begin, sites, init_pos=init_pos)
    want_regions, want_state = A.active_regions(win_begin, depth, cand, anchor)
    d_sites = torch.from_numpy(np.array(sites, np.uint32).reshape(-1).view(np.int64).copy()).cuda()
    d_cand = torch.from_numpy(np.array(cand, np.uint8)).cuda()
    d_anchor = torch.empty(WINDOW, dtype=torch.uint8, device="cuda")
    d_state_in = torch.from_numpy(capi.ar_state_initial().view(np.int32).copy()).cuda()
    d_state_out = torch.empty(6, dtype=torch.int32, device="cuda")
    cap = capi.active_regions_bound(WINDOW)
    d_regions = torch.empty(cap * 3, dtype=torch.int32, device="cuda")
    d_n = torch.empty(1, dtype=torch.int32, device="cuda")

    def ar1():
        capi._check(L.sk_ref_anchors_dev(p(d_ref), OFF, len(ref), init_pos, None, win_begin, WINDOW, p(d_anchor), 0, None, None, st))

    def ar2():
        capi._check(L.sk_active_regions_dev(win_begin, WINDOW, p(d_sites), p(d_cand), p(d_anchor), p(d_state_in), p(d_state_out), p(d_regions), cap, p(d_n), st))

    def both():
        ar1()
        ar2()

    t1, t2, t12 = timed(ar1), timed(ar2), timed(both)
    assert d_anchor.cpu().tolist() == anchor
    n = int(d_n.cpu()[0])
    assert [tuple(int(x) for x in r) for r in d_regions.cpu().numpy().view(capi.ACTIVE_REGION_DTYPE)[:n]] == want_regions
    result[name] = dict(positions=WINDOW, candidates=int(sum(cand)), anchors=int(sum(anchor)), regions=n, ar1_ms=t1, ar2_ms=t2, ar1_ar2_ms=t12)

# the span rows of four positions
span_pos = torch.from_numpy(np.array([OFF, OFF + 3300, OFF + 5000, OFF + WINDOW], np.int32)).cuda()
d_rows = torch.empty(4 * 50, dtype=torch.int32, device="cuda")
t = timed(lambda: capi._check(L.sk_ref_anchors_dev(p(d_ref), OFF, len(ref), OFF + 1, None, OFF, 0, None, 4, p(span_pos), p(d_rows), st)))
assert d_rows.cpu().numpy().astype(np.uint32).reshape(4, 50).tolist() == A.ref_anchors(ref, OFF, OFF + 1, None, OFF, 0, span_pos.cpu().tolist())[1]
result["span_rows_4"] = dict(ms=t)

# AR1 alone on 2^26 positions of a periodic reference
period = ref[500:500 + 4096]
big = 1 << 26
tiles = big // len(period) + 2
d_big = torch.from_numpy(np.tile(np.frombuffer(period.encode(), np.uint8), tiles)).cuda()
d_big_anchor = torch.empty(big, dtype=torch.uint8, device="cuda")
t = timed(lambda: capi._check(L.sk_ref_anchors_dev(p(d_big), 0, len(period) * tiles, 1, None, 0, big, p(d_big_anchor), 0, None, None, st)))
got = d_big_anchor.cpu().numpy()
inner = got[len(period):len(period) * (big // len(period))].reshape(-1, len(period))
assert (inner == inner[0][None, :]).all()
assert got[:6000].tolist() == A.ref_anchors(period * 3, 0, 1, None, 0, 6000)[0]
result["ar1_2^26"] = dict(positions=big, anchors=int(got.sum()), ms=t, positions_per_us=big / t["median"] / 1e3)

# the reference's own finder on one core, timed inside the golden driver
driver = os.path.join("oracle", "_ref", "bin", "active_region_driver")
if os.path.exists(driver):
    lines = ["REF %d %s" % (OFF, ref), "TIME %d %d" % (OFF + 1, WINDOW), "REF 0 " + period * ((1 << 22) // len(period) + 1), "TIME 1 %d" % (1 << 22)]
    out = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
    items = json.loads(out)["items"]
    result["reference_finder_one_core"] = [dict(positions=it["n_head"], ms=it["seconds"] * 1e3, positions_per_us=it["n_head"] / it["seconds"] / 1e6) for it in items]
else:
    result["reference_finder_one_core"] = "not measured (tools/golden/active_region_driver.cpp not built)"
print(json.dumps(result))
