"""time of the synchronised walk (sk_sync_active_regions_dev, AR3, with and without its region_id fill) against S launches of the
single-sample walk (sk_active_regions_dev, AR2) on the same arrays: windows of 8 192 and 16 384 positions, S = 1, 2 and 8, between device
events, in one process, the two alternated after a warm-up.  The samples' counters are seeded independently over one repeat-rich
reference (a few dozen candidates per sample and window, as tools/diag/active_region_bench.py takes them).  Every result is checked
against the models (tests/sync_model.py, tests/anchor_model.py).  usage: python tools/diag/sync_regions_bench.py [reps] -> one JSON line"""
import ctypes as C
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from strelka_amd import capi  # noqa: E402
from tests import active_region_cases as R  # noqa: E402
from tests import anchor_model as A  # noqa: E402
from tests import intake_cases as K  # noqa: E402
from tests import sync_model as S  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
capi.init(0)
L = capi.lib()
OFF = 1000
p = lambda t: C.c_void_p(t.data_ptr())
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def timed_alternately(runs):
    """{name: run} -> {name: spread of milliseconds}: a warm-up of each, then reps rounds of every run in turn"""
    for run in runs.values():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: spread(v) for k, v in ms.items()}


result = {}
for n_pos in (8192, 16384):
    rng = np.random.default_rng(8900 + n_pos)
    ref = K.repeat_rich_reference(n_pos + 1400, rng)
    win_begin = OFF + 1000
    for n_samples in (1, 2, 8):
        sites = [R.walk_sites(n_pos, rng, 0.004) for _ in range(n_samples)]
        flags = [R.walk_flags(ref, OFF, win_begin, s, init_pos=OFF + 1) for s in sites]
        depth, cand, anchor = [f[0] for f in flags], [f[1] for f in flags], flags[0][2]
        want, want_state, want_id = S.sync_active_regions(win_begin, depth, cand, anchor)
        d_sites = torch.from_numpy(np.array(sites, np.uint32).reshape(-1).view(np.int64).copy()).cuda()
        d_cand = torch.from_numpy(np.array(cand, np.uint8).reshape(-1)).cuda()
        d_anchor = torch.from_numpy(np.array(anchor, np.uint8)).cuda()
        mark_off, marks = capi.pack_ploidy_marks(None, n_samples)
        d_mark_off, d_marks = torch.from_numpy(mark_off).cuda(), torch.from_numpy(marks.view(np.int32).copy()).cuda()
        d_state_in = torch.from_numpy(capi.sync_state_initial().view(np.int32).copy()).cuda()
        d_state_out = torch.empty(52, dtype=torch.int32, device="cuda")
        cap = capi.sync_regions_bound(n_pos)
        d_sync = torch.empty(cap * 8, dtype=torch.int32, device="cuda")
        d_n = torch.empty(1, dtype=torch.int32, device="cuda")
        d_id = torch.empty(n_pos, dtype=torch.int32, device="cuda")
        # AR2's own outputs, per sample
        cap2 = capi.active_regions_bound(n_pos)
        d_ar_in = torch.from_numpy(capi.ar_state_initial().view(np.int32).copy()).cuda()
        d_ar_out = torch.empty(6 * n_samples, dtype=torch.int32, device="cuda")
        d_regions = torch.empty(n_samples * cap2 * 3, dtype=torch.int32, device="cuda")
        d_n2 = torch.empty(n_samples, dtype=torch.int32, device="cuda")

        def ar3(with_ids):
            capi._check(L.sk_sync_active_regions_dev(n_samples, win_begin, n_pos, p(d_sites), p(d_cand), p(d_anchor), p(d_mark_off), p(d_marks), 2, p(d_state_in), p(d_state_out),
                                                     0, None, None, p(d_sync), cap, p(d_n), p(d_id) if with_ids else None, st))

        def ar2():
            for s in range(n_samples):
                capi._check(L.sk_active_regions_dev(win_begin, n_pos, p(d_sites[s * n_pos:]), p(d_cand[s * n_pos:]), p(d_anchor), p(d_ar_in), p(d_ar_out[6 * s:]),
                                                    p(d_regions[s * cap2 * 3:]), cap2, p(d_n2[s:]), st))

        t = timed_alternately(dict(ar2_per_sample_launches=ar2, ar3_walk=lambda: ar3(False), ar3_walk_and_region_id=lambda: ar3(True)))
        n = int(d_n.cpu()[0])
        got = d_sync.cpu().numpy()[:n * 8].view(capi.SYNC_REGION_DTYPE)
        assert [(int(g["begin"]), int(g["end"]), int(g["closed_at"]), int(g["prev_end"]), int(g["sample_mask"])) for g in got] == \
            [(w["begin"], w["end"], w["closed_at"], w["prev_end"], w["sample_mask"]) for w in want]
        assert d_id.cpu().tolist() == want_id
        n_own = 0
        for s in range(n_samples):
            own, _ = A.active_regions(win_begin, depth[s], cand[s], anchor)
            k = int(d_n2[s].cpu())
            assert [tuple(int(x) for x in r) for r in d_regions.cpu().numpy()[s * cap2 * 3:].view(capi.ACTIVE_REGION_DTYPE)[:k]] == own
            n_own += k
        result["n_pos_%d_samples_%d" % (n_pos, n_samples)] = dict(candidates=int(np.sum(cand)), anchors=int(sum(anchor)), sample_regions=n_own, synchronised_regions=n, ms=t,
                                                                  ar3_over_ar2=t["ar3_walk"]["median"] / t["ar2_per_sample_launches"]["median"])
print(json.dumps(result))
